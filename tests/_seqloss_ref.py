"""A restatement of speechbrain.nnet.losses.nll_loss / kldiv_loss (1.0) and speechbrain.utils.Accuracy with upstream's own operations
(F.nll_loss, F.kl_div, scatter_, masked_fill, the length mask of length_to_mask), in float64 by default: the reference of
tests/test_seqloss_cpu.py and tests/test_seqloss_gpu.py.  It shares none of the kernels' algebra (no conf / off / constant, no
sum z - V lse).  `dtype=torch.float32` evaluates the same definitions in float32 on the CPU: the floor of the GPU bars.

Also here: the analytic gradients (checked against autograd in the CPU tests), the accuracy, and the batch the GPU tests run."""
import torch
import torch.nn.functional as F


def truncate(predictions, targets, allowed_len_diff=3):
    """upstream `truncate`: cut both to the shorter when they differ by at most allowed_len_diff, ValueError beyond."""
    diff = predictions.shape[1] - targets.shape[1]
    if diff == 0:
        return predictions, targets
    if abs(diff) > allowed_len_diff:
        raise ValueError(f"lengths differ by {abs(diff)} > {allowed_len_diff}")
    if diff < 0:
        return predictions, targets[:, :predictions.shape[1]]
    return predictions[:, :targets.shape[1]], targets


def length_mask(length, B, U):
    """upstream compute_masked_loss: ones when length is None, else length_to_mask(length * U, max_len=U): arange(U) in length's
    dtype < (length * U)[:, None].  -> bool (B, U)."""
    if length is None:
        return torch.ones(B, U, dtype=torch.bool)
    abs_len = length * U
    return torch.arange(U, dtype=abs_len.dtype)[None, :].expand(B, U) < abs_len[:, None]


def _reduce_masked(t, mask, reduction):
    B = t.shape[0]
    if reduction == "mean":
        return t.sum() / mask.sum()
    if reduction == "batchmean":
        return t.sum() / B
    if reduction == "batch":
        return t.reshape(B, -1).sum(1) / mask.reshape(B, -1).sum(1)
    return t


def nll_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, reduction="mean", dtype=torch.float64):
    lp, tg = truncate(log_probabilities, targets, allowed_len_diff)
    lp = lp.to(dtype)
    B, U, V = lp.shape
    mask = length_mask(length, B, U).to(dtype)
    tok = F.nll_loss(lp.transpose(1, -1), tg.long(), reduction="none") * mask
    loss = _reduce_masked(tok, mask, reduction)
    if label_smoothing == 0:
        return loss
    reg = torch.mean(lp.transpose(1, -1), dim=1) * mask
    return -label_smoothing * _reduce_masked(reg, mask, reduction) + (1 - label_smoothing) * loss


def kldiv_pointwise(log_probabilities, targets, label_smoothing, pad_idx=0, dtype=torch.float64):
    """upstream's pointwise tensor (B * U, V) after the pad rows are zeroed, and the ignore mask (B * U)."""
    lp = log_probabilities.to(dtype)
    if lp.dim() == 2:
        lp = lp.unsqueeze(1)
    bz, time, n_class = lp.shape
    tg = targets.long().detach()
    confidence = 1 - label_smoothing
    lp = lp.reshape(-1, n_class)
    tg = tg.reshape(-1)
    with torch.no_grad():
        true_distribution = lp.clone()
        true_distribution.fill_(label_smoothing / (n_class - 1))
        ignore = tg == pad_idx
        tg = tg.masked_fill(ignore, 0)
        true_distribution.scatter_(1, tg.unsqueeze(1), confidence)
    loss = F.kl_div(lp, true_distribution, reduction="none")
    return loss.masked_fill(ignore.unsqueeze(1), 0), ignore


def kldiv_loss(log_probabilities, targets, length=None, label_smoothing=0.0, allowed_len_diff=3, pad_idx=0, reduction="mean",
               dtype=torch.float64):
    if label_smoothing == 0:
        return nll_loss(log_probabilities, targets, length, reduction=reduction, dtype=dtype)
    bz = log_probabilities.shape[0]
    loss, _ = kldiv_pointwise(log_probabilities, targets, label_smoothing, pad_idx, dtype)
    if reduction == "mean":
        return loss.sum().mean()
    if reduction == "batchmean":
        return loss.sum() / bz
    if reduction == "batch":
        return loss.view(bz, -1).sum(1) / length.to(dtype)
    if reduction == "sum":
        return loss.sum()
    return loss


# ---- per row: what the kernels' stages are compared with --------------------------------------------------------------------------
def keep_mask(kind, targets, length, pad_idx):
    """bool (B, U): the rows a loss keeps.  nll (and kldiv without smoothing): the length mask; kldiv: targets != pad_idx."""
    B, U = targets.shape
    if kind == "kldiv":
        return targets != pad_idx
    return length_mask(length, B, U)


def row_losses(kind, lp, targets, length, label_smoothing, pad_idx=0, dtype=torch.float64):
    """(B, U) row losses (0 on dropped rows) of log-probabilities lp (B, U, V), from upstream's operations."""
    lp = lp.to(dtype)
    B, U, V = lp.shape
    if kind == "kldiv":
        pw, _ = kldiv_pointwise(lp, targets, label_smoothing, pad_idx, dtype)
        return pw.sum(-1).view(B, U)
    keep = length_mask(length, B, U)
    tok = F.nll_loss(lp.transpose(1, -1), targets.long(), reduction="none")
    if label_smoothing != 0:
        tok = (1 - label_smoothing) * tok - label_smoothing * torch.mean(lp, dim=2)
    return torch.where(keep, tok, torch.zeros_like(tok))


def target_distribution(kind, targets, V, label_smoothing, dtype=torch.float64):
    """(B, U, V): nll - (1 - e) one-hot + e / V; kldiv - 1 - e at the target, e / (V - 1) elsewhere (scatter_, as upstream)."""
    B, U = targets.shape
    if kind == "kldiv":
        q = torch.full((B, U, V), label_smoothing / (V - 1), dtype=dtype)
        q.scatter_(2, targets.long().unsqueeze(-1), 1 - label_smoothing)
        return q
    q = torch.full((B, U, V), label_smoothing / V, dtype=dtype)
    q.scatter_add_(2, targets.long().unsqueeze(-1), torch.full((B, U, 1), 1 - label_smoothing, dtype=dtype))
    return q


def grad_log_probs(kind, targets, V, keep, g, label_smoothing, dtype=torch.float64):
    """d(sum_bu g row_loss) / d lp = -g keep q."""
    q = target_distribution(kind, targets, V, label_smoothing, dtype)
    return -(g.to(dtype) * keep.to(dtype)).unsqueeze(-1) * q


def grad_logits(kind, z, targets, keep, g, label_smoothing, dtype=torch.float64):
    """d(sum_bu g row_loss(log_softmax z)) / d z = g keep (softmax z - q)   (sum_v q = 1)."""
    z = z.to(dtype)
    q = target_distribution(kind, targets, z.shape[-1], label_smoothing, dtype)
    return (g.to(dtype) * keep.to(dtype)).unsqueeze(-1) * (torch.softmax(z, -1) - q)


def first_argmax(scores):
    """The SMALLEST index among the entries equal to the row maximum (what torch.argmax returns on the CPU for these inputs, stated
    without relying on it)."""
    V = scores.shape[-1]
    top = scores == scores.max(-1, keepdim=True).values
    return torch.where(top, torch.arange(V).expand_as(scores), torch.full_like(top, V, dtype=torch.int64)).min(-1).values


def accuracy(scores, targets, keep):
    """(hits (B), kept (B)) int64: argmax == target over the kept rows."""
    hit = (first_argmax(scores) == targets.long()) & keep
    return hit.sum(1), keep.sum(1)


# ---- the batch of the GPU tests ---------------------------------------------------------------------------------------------------
def rel_lengths(B):
    """Utterance 0 at full length, utterance 1 at a fractional one (0.5 U = 2.5 at U = 5 keeps three steps), utterance 2 with no
    kept step."""
    return torch.tensor([1.0, 0.5, 0.0][:B], dtype=torch.float32)


def case(B, U, V, dtype, seed, scale=2.0, shift=0.0):
    """Logits (B, U, V) rounded to `dtype`, targets, relative lengths and the pad token made on the CPU from a seed.  Where the shape
    has room: token 0 at (0, 0), token V - 1 at (0, U - 1), the pad token inside the kept span at (0, U // 2), and the last
    utterance (B >= 2) all pad - for kldiv an utterance without a kept row; for nll the length mask leaves utterance 2 without one."""
    g = torch.Generator().manual_seed(seed)
    z = (torch.randn(B, U, V, generator=g, dtype=torch.float64) * scale + shift).to(dtype)
    tg = torch.randint(0, V, (B, U), generator=g)
    pad = min(1, V - 1)
    if B >= 2:
        tg[B - 1, :] = pad
    tg[0, 0] = 0
    if U > 1:
        tg[0, U - 1] = V - 1
    if U > 2:
        tg[0, U // 2] = pad
    return z, tg, rel_lengths(B), pad
