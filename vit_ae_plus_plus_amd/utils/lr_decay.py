"""Layer-wise learning-rate decay for fine-tuning the 3-D ViT (reference: utils/lr_decay.py:15-75, after BEiT).

Depth position of a parameter: 0 for the embedding (``cls_token``, ``pos_embed``, ``patch_embed.*``), ``i + 1`` for
``blocks.i.*``, and ``len(blocks) + 1`` for whatever sits above the blocks (``norm`` / ``fc_norm``, ``head``).  A group's
``lr_scale`` is ``layer_decay ** (top - position)``, which ``lr_sched.adjust_learning_rate`` multiplies into the
schedule's learning rate; vectors and the names in ``no_weight_decay_list`` get no weight decay.
"""


def get_layer_id_for_vit(name, num_layers):
    """Depth position of parameter ``name`` in a model with ``num_layers - 1`` blocks."""
    if name in ('cls_token', 'pos_embed') or name.startswith('patch_embed'):
        return 0
    if name.startswith('blocks'):
        return int(name.split('.')[1]) + 1
    return num_layers


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=.75):
    """Optimizer parameter groups, one per (depth position, decayed or not), in order of first appearance among
    ``model.named_parameters()``; frozen parameters are left out."""
    num_layers = len(model.blocks) + 1
    groups = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decayed = p.ndim != 1 and name not in no_weight_decay_list
        layer = get_layer_id_for_vit(name, num_layers)
        key = 'layer_%d_%s' % (layer, 'decay' if decayed else 'no_decay')
        if key not in groups:
            groups[key] = {'lr_scale': layer_decay ** (num_layers - layer),
                           'weight_decay': weight_decay if decayed else 0.,
                           'params': []}
        groups[key]['params'].append(p)
    return list(groups.values())
