"""Training and evaluation loops of the 3-D ResNet baseline (reference k_fold_training_scripts/train_3d_resnet.py:29-97, :100-137,
:196-204) and ``get_all_feat_and_labels``, which the reference's pre-training scripts import from here.

``train_one_epoch``: the fine-tuning loop of ``post_training_utils.fine_tune_epoch`` — same signature, ``(samples, _, targets)`` batches,
``args.accum_iter``, per-iteration schedule, ``mix_up_fn``.
``evaluate``: same signature and keys (``loss``, ``roc_score``, ``spec``, ``sens``); the unweighted cross entropy, the softmax and the
confusion counts of a batch come from ONE ``vitae_cls_loss`` launch and are read back once, after the last batch.

Deviations: no ``main`` (datasets, torchio and the k-fold driver stay with the reference's script); no autocast region — the model's
operands are bf16 by construction, the criterion sees fp32 logits.
"""
import torch

from .._abi import lib
from ..post_training_utils import fine_tune_epoch
from ..utils import misc, used_metrics

train_one_epoch = fine_tune_epoch.train_one_epoch


@torch.no_grad()
def evaluate(data_loader, model, device, args):
    metric_logger = misc.MetricLogger(delimiter="  ")
    model.eval()

    losses, probs, targets, confusion = [], [], [], None
    for batch in metric_logger.log_every(data_loader, 10, 'Test:'):
        images = batch[0].to(device, non_blocking=True)
        target = batch[-1].to(device, non_blocking=True).long().contiguous()
        output = model(images)
        B, C = output.shape
        loss = torch.empty((), dtype=torch.float32, device=output.device)
        p = torch.empty(B, C, dtype=torch.float32, device=output.device)
        pred = torch.empty(B, dtype=torch.int32, device=output.device)
        if confusion is None:
            confusion = torch.zeros(C * C, dtype=torch.int32, device=output.device)
        lib.vitae_cls_loss(output.data_ptr(), output.stride(0), target.data_ptr(), None, None, 1.0, loss.data_ptr(), None, p.data_ptr(),
                           pred.data_ptr(), confusion.data_ptr(), B, C, torch.cuda.current_stream(output.device).cuda_stream)
        losses.append(loss)
        probs.append(p)
        targets.append(target)

    if not losses:
        raise ValueError('evaluate: the data loader produced no batch')
    if probs[0].shape[1] != 2:
        raise ValueError(f'evaluate: the metrics are those of a two-class task, the model has {probs[0].shape[1]} classes')
    # one read-back: [batch losses | confusion counts | softmax column 0 | softmax column 1 | labels], all exact in double
    p_all, y_all = torch.cat(probs), torch.cat(targets)
    host = torch.cat((torch.stack(losses).double(), confusion.double(), p_all.t().reshape(-1).double(), y_all.double())).cpu().numpy()
    n_b, n = len(losses), y_all.shape[0]
    for v in host[:n_b]:
        metric_logger.update(loss=float(v))
    cm = host[n_b:n_b + 4].astype('int64').reshape(2, 2)
    p_host = host[n_b + 4:n_b + 4 + 2 * n].reshape(2, n).T
    label = host[n_b + 4 + 2 * n:].astype('int64')
    used_metrics._check_two_classes(label)
    roc_score = used_metrics._macro_auc(p_host, label)
    spec, sens = used_metrics._rates(cm)
    metric_logger.update(roc_score=roc_score)
    metric_logger.update(spec=spec)
    metric_logger.update(sens=sens)
    metric_logger.synchronize_between_processes()
    print('* acc {:.3f}, loss {losses.global_avg:.3f}'.format(roc_score, losses=metric_logger.loss))
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def get_all_feat_and_labels(dataset_whole, args):
    """Every item's volume and label as two tensors: single-channel volumes are concatenated along their leading axis (as the
    reference does), multi-channel ones stacked."""
    items = [dataset_whole[i] for i in range(len(dataset_whole))]
    volumes, labels = [it[0] for it in items], [it[-1] for it in items]
    join = torch.cat if args.in_channels == 1 else torch.stack
    return join(volumes), torch.stack(labels)
