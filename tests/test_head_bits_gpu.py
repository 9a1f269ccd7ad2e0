"""The bits of the vocabulary-head kernels, pinned: the row passes (ops.ctc_best_path, ops.seqloss_fwd / seqloss_bwd,
ops.log_softmax_fwd, ops.transducer_row_stats), the fused head tiles (ops.ctc_head_best_path, ops.transducer_gemm_stats /
transducer_gemm_grad) and ops.greedy_decode.  The SHA-256 of the raw bytes of every output tensor must equal
tests/golden/head_bits.json, case by case.  The float64 tests of these kernels allow a tolerance and would not see a changed
summation order, a changed merge order of a row's partial (max, sum exp) pairs or another rounding of the fp32 product; this one
does.  Inputs are integer patterns (exact in bf16) with a power-of-two spread, no random generator.  The shapes are the smallest
that reach every branch of the shared code: a last block with one live wave, a tail only / groups and a tail / a partly filled round of
groups in flight / more than one round, aligned rows and rows at an odd element offset of a NaN-filled buffer, a second row tile with two live rows,
a second column tile with four live columns, three column tiles, one K stage and three.
`python tests/test_head_bits_gpu.py --write <path>` writes the fixture (case names and hex digests only)."""
import hashlib
import json
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (for --write: run as a script)
from tests._util import pattern as _pattern  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "head_bits.json")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN, INF = float("nan"), float("inf")
ROWS = 9                                                 # three blocks of four waves: the last block has one live wave
TIE, NEG, ONE_NAN, ALL_NAN = 2, 4, 6, 7                  # the special rows of a row-pass input


def _digest(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _place(x, dtype, layout):
    """x (float64, 2-D, on the host) on the device in dtype: dense, or as the column slice at element offset 3 of a buffer five
    columns wider that is NaN elsewhere (rows at odd element offsets: the element-wise path of the 16-byte group loaders)."""
    x = x.to(dtype).cuda()
    if layout == "dense":
        return x
    buf = torch.full((x.shape[0], x.shape[1] + 5), NAN, dtype=dtype, device="cuda")
    buf[:, 3:3 + x.shape[1]] = x
    return buf[:, 3:3 + x.shape[1]]


def _scores(V, nans):
    """(ROWS, V) scores within +-15; row TIE holds its maximum twice, in two different lanes (the lower column must win); row NEG has
    a -inf column; with nans, row ONE_NAN has one NaN and row ALL_NAN nothing else."""
    x = _pattern(ROWS, V, (37, 11), 61, 16, -3, 7)
    x[TIE, V // 3] = 64.0
    x[TIE, V - 1] = 64.0
    x[NEG, V // 2] = -INF
    if nans:
        x[ONE_NAN, V // 4] = NAN
        x[ALL_NAN, :] = NAN
    return x


def _best_path(dtype, V, layout):
    from summarymixing_amd import ops
    return ops.ctc_best_path(_place(_scores(V, True), dtype, layout))


def _seqloss(dtype, V, layout, from_logits, smooth):
    from summarymixing_amd import ops
    B, U = 3, 3
    x = _place(_scores(V, False), dtype, layout).unflatten(0, (B, U))
    tgt = ((5 * torch.arange(ROWS) + 1) % V).to(torch.int32)
    tgt[TIE] = V // 3                                    # the row's arg-max: a hit
    tgt = tgt.view(B, U).cuda()
    keep = torch.tensor([3, 3, 2], dtype=torch.int32, device="cuda")        # the last row is dropped
    s = 0.125 if smooth else 0.0
    conf, off = 1.0 - s, s / (V - 1)
    cst = conf * math.log(conf) + (V - 1) * off * math.log(off) if smooth else 0.0
    row_loss, lse, flags, utt_loss, utt_kept, utt_hits = ops.seqloss_fwd(x, tgt, keep, -1, conf, off, cst, from_logits)
    g = (_pattern(B, U, (3, 5), 13, 8, -2, 3) + 1.0).float().cuda().contiguous()
    dx = ops.seqloss_bwd(x, tgt, keep, -1, conf, off, lse, g, from_logits)
    outs = [row_loss, flags, utt_loss, utt_kept, utt_hits, dx]
    return outs + ([lse] if from_logits else [])


def _log_softmax(dtype, V, layout):
    from summarymixing_amd import ops
    return [ops.log_softmax_fwd(_place(_scores(V, False), dtype, layout))]


def _row_stats(dtype, V, layout):
    from summarymixing_amd import ops
    B, T, U1 = 1, 3, 3
    tgt = ((torch.arange(U1 - 1) + 1) % V).to(torch.int32).view(B, U1 - 1).cuda()
    return ops.transducer_row_stats(_place(_scores(V, False), dtype, layout), tgt, B, T, U1, 0)


N_HEAD = 130                                             # a second row tile with two live rows


def _head_operands(dtype, K, V, bias):
    """Exponents over 13 octaves per operand: the products (exact in fp32) span 25 octaves, so an fp32 sum over K rounds - a forward
    chain, its reverse and the two-level sum of 32-element stages differ in a third to two thirds of the 130 x V entries at K = 64
    and 192 (checked on the host), with |z| <= 9.  The six-octave spread of the row inputs would leave every partial sum exact."""
    x = _pattern(N_HEAD, K, (37, 11), 61, 16, -12, 13).to(dtype).cuda()
    w = _pattern(V, K, (13, 29), 53, 16, -12, 13).to(dtype).cuda()
    b = _pattern(1, V, (0, 7), 31, 8, -2, 3).float().view(V).cuda() if bias else None
    return x, w, b


def _ctc_head(dtype, K, V, bias):
    from summarymixing_amd import ops
    x, w, b = _head_operands(dtype, K, V, bias)
    assert ops.ctc_head_ok(dtype, K, V)
    return ops.ctc_head_best_path(x, w, b)


def _transducer_head(dtype, J, V, bias):
    """Forward statistics, then the gradient twice: all rows with the second row tile's two rows without a gradient (the tile
    stores zeros and skips the product), and rows [1, 130) with a gradient in every row."""
    from summarymixing_amd import ops
    B, T, U1, blank = 2, 5, 13, 1
    assert B * T * U1 == N_HEAD and ops.transducer_fused_ok(dtype, J, V)
    h, w, b = _head_operands(dtype, J, V, bias)
    bb = torch.arange(B).view(-1, 1)
    uu = torch.arange(U1 - 1).view(1, -1)
    tgt = (128 + (7 * bb + 3 * uu) % (V - 128)).to(torch.int32).cuda()      # the blank in column tile 0, every label beyond it
    lse, lpb, lpy = ops.transducer_gemm_stats(h, w, b, tgt, B, T, U1, blank)
    gb = -(_pattern(1, N_HEAD, (0, 5), 17, 64, -1, 3).abs() + 2.0 ** -7).float().view(N_HEAD)
    gy = -(_pattern(1, N_HEAD, (0, 3), 19, 64, -1, 3).abs() + 2.0 ** -7).float().view(N_HEAD)
    gb0, gy0 = gb.clone(), gy.clone()
    gb0[128:] = 0.0
    gy0[128:] = 0.0
    dz0 = torch.empty((N_HEAD, V), dtype=dtype, device="cuda")
    ops.transducer_gemm_grad(h, w, b, tgt, lse, gb0.cuda(), gy0.cuda(), B, T, U1, blank, 0, N_HEAD, dz0)
    dz1 = torch.empty((N_HEAD - 1, V), dtype=dtype, device="cuda")
    ops.transducer_gemm_grad(h, w, b, tgt, lse, gb.cuda(), gy.cuda(), B, T, U1, blank, 1, N_HEAD - 1, dz1)
    return [lse, lpb, lpy, dz0, dz1]


def _greedy(dtype):
    """The smallest shape smx_greedy_ok accepts: three rows of a 16-row tile, two vocabulary tiles."""
    from summarymixing_amd import _lib, ops
    B, T, V, H, J, blank = 3, 4, 130, 32, 64, 0
    assert ops.greedy_ok(dtype, H, J, V)
    enc = _pattern(B * T, J, (37, 11), 61, 16, -8, 9).to(dtype).cuda().view(B, T, J)
    WihT = _pattern(V - 1, 4 * H, (13, 7), 41, 32, -2, 3).to(dtype).cuda()
    Whh = _pattern(4 * H, H, (11, 17), 43, 32, -3, 3).to(dtype).cuda()
    Wproj = _pattern(J, H, (19, 5), 37, 16, -2, 3).to(dtype).cuda()
    Wlin = _pattern(V, J, (13, 29), 53, 16, -8, 9).to(dtype).cuda()
    bias = _pattern(1, 4 * H, (0, 5), 17, 8, -1, 2).float().view(4 * H).cuda()
    blin = _pattern(1, V, (0, 7), 31, 8, -1, 2).float().view(V).cuda()
    state = ops.greedy_start(bias, Wproj, B)
    logp = torch.zeros(B, dtype=torch.float32, device="cuda")
    tokens, frames, n_tok = ops.greedy_decode(enc, None, WihT, bias, Whh, Wproj, Wlin, blin, state, logp, _lib.ACT_RELU, blank)
    return [tokens, frames, n_tok, logp, state[0], state[1]]


def _cases():
    cases = {}
    for dn, dtype in DTYPES.items():
        for layout in ("dense", "offset"):
            # a tail only / groups and a tail / a partly filled round of groups in flight / a second round (2100 > 64 lanes x 4
            # groups x 8 bf16; three rounds in fp32)
            for V in (2, 65, 300, 1003, 2100):
                cases[f"ctc_best_path-{dn}-V{V}-{layout}"] = (_best_path, (dtype, V, layout))
                for form in ("logits", "logprobs"):
                    for smooth in (False, True):
                        cases[f"seqloss-{form}-{'smooth' if smooth else 'plain'}-{dn}-V{V}-{layout}"] = \
                            (_seqloss, (dtype, V, layout, form == "logits", smooth))
            for V in (2, 65, 1000):
                cases[f"log_softmax-{dn}-V{V}-{layout}"] = (_log_softmax, (dtype, V, layout))
                cases[f"transducer_row_stats-{dn}-V{V}-{layout}"] = (_row_stats, (dtype, V, layout))
        for V in (132, 300):                             # four live columns in a second column tile / three column tiles
            for K in (64, 192):                          # one K stage / a steady-state prefetch (bf16; fp32: two and six)
                for bias in (False, True):
                    tail = f"{dn}-V{V}-K{K}-{'bias' if bias else 'nobias'}"
                    cases[f"ctc_head-{tail}"] = (_ctc_head, (dtype, K, V, bias))
                    cases[f"transducer_head-{tail}"] = (_transducer_head, (dtype, K, V, bias))
        cases[f"greedy-{dn}"] = (_greedy, (dtype,))
    return cases


CASES = _cases()


def _run(name):
    fn, args = CASES[name]
    return [_digest(t) for t in fn(*args)]


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_head_bits_equal_the_fixture(name, golden):
    got, want = _run(name), golden[name]
    assert len(got) == len(want), f"{name}: {len(got)} outputs, the fixture has {len(want)}"
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, f"{name}: the bits of output {i} differ from the fixture"


def test_fixture_has_exactly_these_cases(golden):
    assert sorted(golden) == sorted(CASES)


def test_fixture_sees_the_fp32_rounding_of_the_head_product(golden):
    """bf16 and fp32 runs of a fused head read the same operand values; their results can differ only where the fp32 sum over K
    rounds (x16 MFMA chain against two-level x2 sums).  If the digests agreed, the inputs would not show the summation order."""
    for name in CASES:
        if name.startswith(("ctc_head-f32", "transducer_head-f32")):
            a, b = golden[name], golden[name.replace("-f32-", "-bf16-")]
            assert a[1] != b[1], f"{name}: fp32 and bf16 give the same bits, the inputs do not make the product round"


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_head_bits_gpu.py --write <path>")
    with open(sys.argv[2], "w") as f:
        json.dump({name: _run(name) for name in sorted(CASES)}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(CASES)} cases to {sys.argv[2]}")
