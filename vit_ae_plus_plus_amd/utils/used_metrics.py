"""Metrics of the two-class fine-tuning task (reference utils/used_metrics.py:12-41) without scikit-learn.

``roc_auc(predictions, target) -> (auc, specificity, sensitivity)``, ``find_vals`` and ``acc_pred`` take raw scores
``[n, 2]`` and class indices ``[n]`` and return the reference's values:

* the AUC is sklearn's macro ``roc_auc_score(one_hot(target), softmax(predictions))``: per softmax column the rank statistic
  (sum of the positives' ranks - n_pos (n_pos + 1) / 2) / (n_pos n_neg) with average ranks for ties — the area under the ROC
  curve sklearn integrates — and the mean of the two columns.  The softmax is torch's fp32 one, as in the reference, so the
  same scores tie;
* specificity and sensitivity are read off the 2 x 2 counts ``cm[pred, label]`` — the reference calls
  ``confusion_matrix(predictions, target)``, predictions first — as ``cm[0, 0] / (cm[0, 0] + cm[1, 0])`` and
  ``cm[1, 1] / (cm[1, 1] + cm[0, 1])``; a zero denominator gives NaN, as numpy gives the reference.

A target with one class only (or a label other than 0 / 1) raises ``ValueError``, as sklearn does.  Device tensors are
accepted and brought to the host in one copy.  Deviation: the reference's debugging ``print`` calls are not reproduced.
"""
import numpy as np
import torch


def _to_host(predictions, target):
    """-> (scores fp32 [n, C] CPU tensor, labels int64 [n] numpy) with ONE device-to-host copy."""
    predictions, target = torch.as_tensor(predictions), torch.as_tensor(target)
    if predictions.dim() != 2 or target.dim() != 1 or target.shape[0] != predictions.shape[0]:
        raise ValueError(f'expected scores [n, classes] and labels [n], got {tuple(predictions.shape)} and {tuple(target.shape)}')
    if predictions.is_cuda or target.is_cuda:
        # labels are small integers: exact in the scores' fp32
        both = torch.cat((predictions.detach().float(), target.detach().to(predictions.device).float()[:, None]), dim=1).cpu()
        return both[:, :-1].contiguous(), both[:, -1].numpy().astype(np.int64)
    return predictions.detach().float(), target.detach().numpy().astype(np.int64)


def _counts(pred, label):
    """cm[p, l] = number of samples with argmax p and label l, over the classes 0 / 1."""
    cm = np.zeros((2, 2), dtype=np.int64)
    np.add.at(cm, (pred, label), 1)
    return cm


def _rates(cm):
    """(specificity, sensitivity) of the 2 x 2 counts cm[pred, label]; 0 / 0 = NaN."""
    with np.errstate(divide='ignore', invalid='ignore'):
        specificity = np.float64(cm[0, 0]) / np.float64(cm[0, 0] + cm[1, 0])
        sensitivity = np.float64(cm[1, 1]) / np.float64(cm[1, 1] + cm[0, 1])
    return float(specificity), float(sensitivity)


def _check_two_classes(label):
    if label.size == 0 or label.min() < 0 or label.max() > 1:
        raise ValueError('labels must be 0 or 1')
    if label.min() == label.max():
        raise ValueError('Only one class present in target. ROC AUC score is not defined in that case.')


def _average_ranks(s):
    _, inv, cnt = np.unique(s, return_inverse=True, return_counts=True)
    end = np.cumsum(cnt)
    return ((end - cnt + 1 + end) / 2.0)[inv.reshape(-1)]


def _macro_auc(probs, label):
    """probs [n, 2] (numpy), label [n] in {0, 1} with both present."""
    aucs = []
    for k in (0, 1):
        pos = label == k
        n_pos, n_neg = int(pos.sum()), int((~pos).sum())
        ranks = _average_ranks(np.asarray(probs[:, k], dtype=np.float64))
        aucs.append((ranks[pos].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))
    return float(np.mean(aucs))


def _argmax(scores):
    return torch.max(scores, dim=1)[1].numpy()


def roc_auc(predictions, target):
    scores, label = _to_host(predictions, target)
    _check_two_classes(label)
    if scores.shape[1] != 2:
        raise ValueError(f'two-class scores expected, got {scores.shape[1]} columns')
    specificity, sensitivity = _rates(_counts(_argmax(scores), label))
    return _macro_auc(torch.softmax(scores, dim=1).numpy(), label), specificity, sensitivity


def acc_pred(predictions, target):
    scores, label = _to_host(predictions, target)
    return torch.tensor(int((_argmax(scores) == label).sum())) / label.shape[0]


def find_vals(predictions, target):
    scores, label = _to_host(predictions, target)
    if scores.shape[1] != 2 or label.size == 0 or label.min() < 0 or label.max() > 1:
        raise ValueError('two-class scores and labels 0 / 1 expected')
    return _rates(_counts(_argmax(scores), label))
