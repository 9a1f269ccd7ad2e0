"""The streaming kernels on the GPU: smx_stream_summary against a float64 restatement of the DynChunk window mean, and
smx_dwconv1d_glu_stream chained over whole sequences against the full-sequence Dynamic Chunk Convolution (ops.dwconv_fwd).
Both are bit-identical across runs."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _chunks(T, C):
    return [(t0, min(T, t0 + C)) for t0 in range(0, T, C)]


def _run_summary(S, B, T, C, left, D):
    from summarymixing_amd import ops
    dev = S.device
    ring = (torch.zeros((B, D), device=dev) if left is None else torch.zeros((B, max(left, 1), D), device=dev))
    counter = torch.zeros(1, dtype=torch.int64, device=dev)
    outs = []
    for t0, t1 in _chunks(T, C):
        s = S[:, t0:t1].reshape(B * (t1 - t0), D)
        out = torch.empty_like(s)
        ops.stream_summary(s, out, B, t1 - t0, C, left, ring, counter)
        ops.step_counter_add(counter, 1)
        outs.append(out.view(B, t1 - t0, D))
    return torch.cat(outs, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("left", [0, 1, 2, 32, None])
@pytest.mark.parametrize("C", [1, 8, 16, 32])
def test_stream_summary_window_mean(C, left, dtype):
    torch.manual_seed(C * 7 + (left or 0))
    B = 3
    nfull = 36 if left == 32 else 7                 # (left 32: the ring wraps)
    T = nfull * C + max(1, C // 2) if C > 1 else nfull
    for D in (144, 512, 1024):
        S = torch.randn(B, T, D, device="cuda").to(dtype)
        out = _run_summary(S, B, T, C, left, D)
        s64 = S.double().cpu()
        ref = torch.empty_like(s64)
        for t0, t1 in _chunks(T, C):
            c = t0 // C
            lo = 0 if left is None else max(0, (c - left) * C)
            ref[:, t0:t1] = s64[:, lo:t1].mean(1, keepdim=True)
        o = out.double().cpu()
        if dtype == torch.float32:
            assert (o - ref).abs().max() <= 1e-5 * ref.abs().max(), (D, (o - ref).abs().max())
        else:                                        # one bf16 ulp of the output
            assert ((o - ref).abs() <= 2.0 ** -8 * ref.abs() + 1e-6).all(), (D, (o - ref).abs().max())
        assert torch.equal(out, _run_summary(S, B, T, C, left, D)), "not bit-reproducible"


def _run_dwconv(P, w, bias, B, T, C, D, k):
    from summarymixing_amd import ops
    state = torch.zeros((B, (k - 1) // 2, 2 * D), dtype=P.dtype, device=P.device)
    outs = []
    for t0, t1 in _chunks(T, C):
        p = P[:, t0:t1].reshape(B * (t1 - t0), 2 * D)
        outs.append(ops.dwconv_stream(p, w, bias, state, B, t1 - t0, D, k).view(B, t1 - t0, D))
    return torch.cat(outs, 1), state


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("C", [4, 8, 15, 16, 32, 64])
def test_dwconv_stream_matches_dynamic_chunk_convolution(C, dtype):
    from summarymixing_amd import _lib as L
    from summarymixing_amd import ops
    torch.manual_seed(C)
    B, k = 2, 31
    H = (k - 1) // 2
    T = 4 * C + max(1, C // 3)
    for D in (144, 256, 512):
        P = torch.randn(B, T, 2 * D, device="cuda").to(dtype)
        w = torch.randn(D, k, device="cuda") * 0.2
        bias = torch.randn(D, device="cuda") * 0.1
        y, state = _run_dwconv(P, w, bias, B, T, C, D, k)
        ref = ops.dwconv_fwd(P.reshape(B * T, 2 * D), w, bias, B, T, D, k, True, L.PAD_ZERO, C).view(B, T, D)
        # fp32 rounding of the tap sum: relative to the sum of |terms|
        p64 = P.double()
        u = p64[..., :D] * torch.sigmoid(p64[..., D:])
        scale = (u.abs().amax() * w.abs().sum(1).max() + bias.abs().max()).item()
        diff = (y.double() - ref.double()).abs()
        if dtype == torch.float32:
            assert diff.max() <= 1e-5 * scale, (D, diff.max())
        else:
            assert (diff <= 2.0 ** -7 * ref.double().abs() + 1e-5 * scale).all(), (D, diff.max())
        # the state is the last H pre-GLU rows of the sequence
        assert torch.equal(state, P[:, T - H:])
        y2, _ = _run_dwconv(P, w, bias, B, T, C, D, k)
        assert torch.equal(y, y2), "not bit-reproducible"


def test_dwconv_stream_other_kernel_sizes():
    """Odd k up to 63 (the full-sequence kernel stops at 33: compared with a float64 restatement)."""
    torch.manual_seed(1)
    B, D, C = 2, 64, 8
    T = 5 * C + 3
    for k in (1, 3, 63):
        H = (k - 1) // 2
        P = torch.randn(B, T, 2 * D, device="cuda")
        w = torch.randn(D, k, device="cuda") * 0.2
        bias = torch.randn(D, device="cuda") * 0.1
        y, _ = _run_dwconv(P, w, bias, B, T, C, D, k)
        p64 = P.double().cpu()
        u = p64[..., :D] * torch.sigmoid(p64[..., D:])
        ref = torch.zeros(B, T, D, dtype=torch.float64)
        for t in range(T):
            lim = min(T, (t // C + 1) * C)
            for j in range(k):
                tau = t + j - H
                if 0 <= tau < lim:
                    ref[:, t] += w[:, j].double().cpu() * u[:, tau]
        ref += bias.double().cpu()
        assert (y.double().cpu() - ref).abs().max() <= 1e-5 * ref.abs().max(), k
