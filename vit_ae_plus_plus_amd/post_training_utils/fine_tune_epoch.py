"""One epoch of supervised fine-tuning of ``VisionTransformer3D`` (reference: post_training_utils/fine_tune_epoch.py:34-100).

Same signature, batch layout ``(samples, _, targets)``, gradient accumulation over ``args.accum_iter`` iterations,
per-iteration learning-rate schedule, exit on a non-finite loss and returned statistics (``loss``, ``lr``).  The reference
wraps the forward in ``torch.cuda.amp.autocast()``; here the arithmetic of the model is chosen by the model's ``precision``
(``model.set_precision('bf16')`` is the counterpart), so no autocast region is opened: the criterion sees fp32 logits.
``evaluate()`` and its metrics are not part of this module.
"""
import math
import sys

import torch

from ..utils import lr_sched, misc


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
