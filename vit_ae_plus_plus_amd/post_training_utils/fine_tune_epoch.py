"""Supervised fine-tuning of ``VisionTransformer3D``: one training epoch, evaluation and checkpoint selection (reference:
post_training_utils/fine_tune_epoch.py:34-100, :104-145, :441-463).

``train_one_epoch``: same signature, batch layout ``(samples, _, targets)``, gradient accumulation over ``args.accum_iter``
iterations, per-iteration learning-rate schedule, exit on a non-finite loss and returned statistics (``loss``, ``lr``).

``evaluate``: same signature and returned keys (``loss``, ``roc_auc_score``, ``specificity``, ``sensitivity``).  Each batch
goes through the inference encoder and the head, then ONE ``vitae_cls_loss`` launch (hard labels, ``args.cross_entropy_wt``)
that leaves the batch loss, the softmax, the argmax and the confusion counts on the device; the losses are read back once,
after the last batch, and fed to the ``MetricLogger`` in order, so ``loss`` is the mean of the batch losses as in the
reference.  The AUC is the rank statistic of ``utils.used_metrics`` on those softmax columns, specificity and sensitivity come
from the confusion counts.

``select_best_model`` / ``evaluate_best_val_model``: the reference's, on ``misc.save_model``; the checkpoint directory comes
from ``args`` (``output_dir``, or ``eval_model_path`` with ``mode='test'``), not from an ``environment_setup`` import.

Deviations: the reference wraps the forwards in ``torch.cuda.amp.autocast()``; here the arithmetic of the model is chosen by
the model's ``precision`` (``model.set_precision('bf16')`` is the counterpart), so no autocast region is opened: the criterion
sees fp32 logits.  The debugging ``print`` calls of the reference's metrics are not reproduced.
"""
import math
import os
import sys

import torch

from .._abi import lib
from ..utils import lr_sched, misc, used_metrics


def train_one_epoch(model, criterion, data_loader, optimizer, device, epoch, loss_scaler,
                    max_norm=0, log_writer=None, args=None, mix_up_fn=None):
    model.train(True)
    metric_logger = misc.MetricLogger(delimiter="  ")
    metric_logger.add_meter('lr', misc.SmoothedValue(window_size=1, fmt='{value:.6f}'))
    header = 'Epoch: [{}]'.format(epoch)
    print_freq = 20
    accum_iter = args.accum_iter
    n_iter = len(data_loader)

    optimizer.zero_grad()
    if log_writer is not None:
        print('log_dir: {}'.format(log_writer.log_dir))

    for step, (samples, _, targets) in enumerate(metric_logger.log_every(data_loader, print_freq, header)):
        last_of_group = (step + 1) % accum_iter == 0
        if step % accum_iter == 0:       # the schedule advances per iteration, in fractional epochs
            lr_sched.adjust_learning_rate(optimizer, step / n_iter + epoch, args)

        samples = samples.to(device, non_blocking=True)
        targets = targets.to(device, non_blocking=True)
        if mix_up_fn is not None:
            samples, targets = mix_up_fn(samples, targets)

        outputs = model(samples)
        loss = criterion(outputs, targets)

        loss_value = loss.item()
        if not math.isfinite(loss_value):
            print("Loss is {}, stopping training".format(loss_value))
            sys.exit(1)

        loss = loss / accum_iter
        loss_scaler(loss, optimizer, clip_grad=max_norm, parameters=model.parameters(), create_graph=False,
                    update_grad=last_of_group)
        if last_of_group:
            optimizer.zero_grad()

        if torch.cuda.is_available():
            torch.cuda.synchronize()

        metric_logger.update(loss=loss_value)
        lrs = [group["lr"] for group in optimizer.param_groups]
        max_lr = max([0.] + lrs)
        metric_logger.update(lr=max_lr)

        loss_value_reduce = misc.all_reduce_mean(loss_value)
        if log_writer is not None and last_of_group:
            # x axis in 1/1000 epochs, so that curves of different batch sizes line up
            epoch_1000x = int((step / n_iter + epoch) * 1000)
            log_writer.add_scalar('loss', loss_value_reduce, epoch_1000x)
            log_writer.add_scalar('lr', max_lr, epoch_1000x)

    metric_logger.synchronize_between_processes()
    print("Averaged stats:", metric_logger)
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


@torch.no_grad()
def evaluate(data_loader, model, device, args):
    weight = getattr(args, 'cross_entropy_wt', None)
    if weight is not None:
        weight = torch.as_tensor(weight).detach().to(device=device, dtype=torch.float32).contiguous()
    metric_logger = misc.MetricLogger(delimiter="  ")
    header = 'Test:'

    # switch to evaluation mode
    model.eval()

    losses, probs, targets, confusion = [], [], [], None
    for batch in metric_logger.log_every(data_loader, 10, header):
        images = batch[0].to(device, non_blocking=True)
        target = batch[-1].to(device, non_blocking=True)

        output = model(images)                     # inference path: refuses tensors that are not on the device
        B, C = output.shape
        if weight is not None and weight.numel() != C:
            raise ValueError(f'args.cross_entropy_wt has {weight.numel()} entries for {C} classes')
        target = target.long().contiguous()
        loss = torch.empty((), dtype=torch.float32, device=output.device)
        p = torch.empty(B, C, dtype=torch.float32, device=output.device)
        pred = torch.empty(B, dtype=torch.int32, device=output.device)
        if confusion is None:
            confusion = torch.zeros(C * C, dtype=torch.int32, device=output.device)
        lib.vitae_cls_loss(output.data_ptr(), output.stride(0), target.data_ptr(), None,
                           None if weight is None else weight.data_ptr(), 1.0, loss.data_ptr(), None, p.data_ptr(), pred.data_ptr(),
                           confusion.data_ptr(), B, C, torch.cuda.current_stream(output.device).cuda_stream)
        losses.append(loss)
        probs.append(p)
        targets.append(target)

    if not losses:
        raise ValueError('evaluate: the data loader produced no batch')
    C = probs[0].shape[1]
    if C != 2:
        raise ValueError(f'evaluate: the metrics are those of a two-class task, the model has {C} classes')
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
    roc_auc_score = used_metrics._macro_auc(p_host, label)
    specificity, sensitivity = used_metrics._rates(cm)
    metric_logger.update(roc_auc_score=roc_auc_score)
    metric_logger.update(specificity=specificity)
    metric_logger.update(sensitivity=sensitivity)
    # gather the stats from all processes
    metric_logger.synchronize_between_processes()
    print('* roc_auc_score {:.3f}, loss {losses.global_avg:.3f}'.format(roc_auc_score, losses=metric_logger.loss))
    return {k: meter.global_avg for k, meter in metric_logger.meters.items()}


def evaluate_best_val_model(args, data_loader_test, dataset_test, device, model, model_name='best_ft_model', mode=None):
    directory = args.eval_model_path if mode == 'test' else args.output_dir
    checkpoint = torch.load(os.path.join(directory, f'checkpoint-{model_name}.pth'), map_location='cpu', weights_only=False)
    model.load_state_dict(checkpoint['model'])
    model.to(device)
    test_stats = evaluate(data_loader=data_loader_test, model=model, device=device, args=args)
    print(f"Accuracy of {model_name} on the {len(dataset_test)} test images: {test_stats['roc_auc_score']:.1f}%")
    return test_stats['roc_auc_score']


def select_best_model(args, epoch, loss_scaler, max_val, model, model_without_ddp, optimizer, cur_val,
                      model_name='best_ft_model'):
    if cur_val > max_val:
        print(f"saving {model_name} @ epoch {epoch}")
        max_val = cur_val
        misc.save_model(args=args, model=model, model_without_ddp=model_without_ddp, optimizer=optimizer,
                        loss_scaler=loss_scaler, epoch=model_name)      # the model's name stands in for the epoch number
    return max_val
