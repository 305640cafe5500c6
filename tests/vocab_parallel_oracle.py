"""Float64 oracle of the vocabulary cross-entropy, computed on FULL rows in numpy and sliced per
shard afterwards: what every rank of a vocabulary-parallel loss must reproduce from its columns.

    loss    = scale / max(1, #rows whose label != ignore_index) * sum_r rowloss[r]
    rowloss = lse(z[r]) - z[r, label[r]]      0 for an ignored or out-of-range label
    grad    = (softmax(z[r]) - onehot(label[r])) * scale / n       a zero row where rowloss is 0

-inf logits are allowed (softmax 0 there); a row needs one finite logit."""
import numpy as np


def full_ce(z, labels, ignore_index=-100, scale=1.0):
    """-> (loss, rowloss [R], grad [R, V]) in float64."""
    z = np.asarray(z, dtype=np.float64)
    lab = np.asarray(labels, dtype=np.int64)
    R, V = z.shape
    m = z.max(axis=1, keepdims=True)
    e = np.exp(z - m)
    lse = m[:, 0] + np.log(e.sum(axis=1))
    valid = (lab != ignore_index) & (lab >= 0) & (lab < V)
    n = max(1, int((lab != ignore_index).sum()))
    safe = np.where(valid, lab, 0)
    rows = np.arange(R)
    rowloss = np.where(valid, lse - z[rows, safe], 0.0)
    grad = np.exp(z - lse[:, None])
    grad[rows[valid], lab[valid]] -= 1.0
    grad *= (valid * (scale / n))[:, None]
    return scale * rowloss.sum() / n, rowloss, grad


def shard(a, bounds, t):
    """Columns [bounds[t], bounds[t + 1]) of a [R, V] array."""
    return a[:, bounds[t]:bounds[t + 1]]
