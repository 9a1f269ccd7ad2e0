"""Thin torch-tensor wrappers over the C-ABI of libsmx.so.

torch is plumbing here: tensors own device memory, ``data_ptr()`` / strides / the current HIP stream are
handed to the kernels.  All arithmetic happens in the hand-written gfx950 kernels.  Matrices are 2-D
views ``(rows, cols)`` with unit stride along cols; the row stride is the leading dimension.
"""
import collections
import ctypes


import torch

from . import _lib as L

_DT = {torch.float32: L.F32, torch.bfloat16: L.BF16}
NO_CPU = "summarymixing_amd kernels run on the GPU only (no CPU fallback)"


def dt(t):
    try:
        return _DT[t.dtype]
    except KeyError:
        raise TypeError(f"summarymixing_amd supports float32 and bfloat16 activations, got {t.dtype}")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# ---- in-step kernel timing (bench.py's roofline_kernels): while `_PROF` is a list every wrapper below brackets its
# launch with two HIP events on the stream it launches on (the wgrad slabs run on a side stream) and appends
# (kernel family + shape, algorithmic bytes, flops, start, end).  Off (None) in normal operation: one `is None` test.
_PROF = None


def prof_start():
    global _PROF
    _PROF = []


def prof_stop(symbols=False):
    """-> list of (name, algorithmic bytes, flops, milliseconds); synchronises the device.  symbols=True: a fifth field, the
    kernel symbol as a profiler prints it (GEMMs: the instantiation smx_gemm_plan_query reports; other launches: their family)."""
    global _PROF
    recs, _PROF = _PROF, None
    torch.cuda.synchronize()
    if symbols:
        return [(r[0], r[1], r[2], r[3].elapsed_time(r[4]), r[5] if len(r) > 5 and r[5] else r[0].split(" (")[0].split(" dW")[0]) for r in recs]
    return [(r[0], r[1], r[2], r[3].elapsed_time(r[4])) for r in recs]


def _pb(name, nbytes, flops=0.0, sym=None):
    if _PROF is None:
        return None
    st = torch.cuda.current_stream()
    e0 = torch.cuda.Event(enable_timing=True)
    e0.record(st)
    return (name, float(nbytes), float(flops), e0, st, sym)


def _pe(tok):
    if tok is not None:
        e1 = torch.cuda.Event(enable_timing=True)
        e1.record(tok[4])
        _PROF.append(tok[:4] + (e1, tok[5]))


def _es(t):
    return 2 if t.dtype == torch.bfloat16 else 4


def _mat(t):
    """(ptr, ld) of a 2-D view with unit inner stride."""
    assert t.dim() == 2 and (t.shape[1] == 1 or t.stride(1) == 1), f"need a (rows, cols) view with unit col stride, got {t.shape} {t.stride()}"
    assert t.is_cuda, NO_CPU
    return _p(t), (t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))


def rows2d(x):
    """(B,T,D) or (N,D) -> (N,D) view without copying (rows must be uniformly strided)."""
    if x.dim() == 2:
        return x
    assert x.dim() == 3
    B, T, D = x.shape
    if x.stride(2) != 1 and D > 1:
        x = x.contiguous()
    if B > 1 and x.stride(0) != T * x.stride(1):
        x = x.contiguous()
    return x.as_strided((B * T, D), (x.stride(1), 1), x.storage_offset()) if T * B > 0 else x.reshape(B * T, D)


def epilogue(bias=None, c0=None, c0_mode=L.C0_NONE, c0_div=0, act=L.ACT_NONE, out_mode=L.OUT_T, z=None,
             row_mask=None, res=None, alpha=1.0, bias_batch_stride=0, drop=None, c0_post=False, act_grad_z=None,
             colsum=None, ln_bwd=None, ln_fwd=None, drop_cols=0, ln_fwd2=None):
    """Build an smx_epilogue.  act_grad_z: the saved pre-activation of the UPSTREAM layer (SMX_EPI_ACT_GRAD: the GEMM
    then emits alpha * D(acc * act'(z)) * mask, i.e. the upstream dZ); colsum: fp32 [M] accumulator of the output's
    column sums (the upstream bias gradient), workspace attached by gemm()."""
    e = L.Epilogue()
    e.epoch = _epoch()                # (the device step counter of the training loop, or NULL: set_step_counter below)
    e.bias = bias.data_ptr() if bias is not None else None
    e.bias_batch_stride = bias_batch_stride
    if c0 is not None:
        assert c0.dtype == torch.float32
        e.c0, e.ldc0 = _mat(c0)
        e.c0 = c0.data_ptr()
        e.c0_mode, e.c0_div = c0_mode, c0_div
    e.act, e.out_mode = act, out_mode
    if z is not None:
        e.z, e.ldz = z.data_ptr(), _mat(z)[1]
    if row_mask is not None:
        assert row_mask.dtype == torch.uint8
        e.row_mask = row_mask.data_ptr()
    if res is not None:
        e.res, e.ldr = res.data_ptr(), _mat(res)[1]
        if res.dtype == torch.float32 and out_mode == L.OUT_F32:
            e.io_flags |= L.IO_RES_F32                   # fp32 residual stream next to bf16 operands
    e.alpha = alpha
    e.flags = L.EPI_C0_POST if c0_post else 0
    if act_grad_z is not None:
        assert z is None and res is None
        e.z, e.ldz = act_grad_z.data_ptr(), _mat(act_grad_z)[1]
        e.flags |= L.EPI_ACT_GRAD
    if colsum is not None:
        assert colsum.dtype == torch.float32 and colsum.is_contiguous()
        e.colsum = colsum.data_ptr()
    if drop is not None and drop[0] > 0.0:
        e.drop_p, e.drop_seed = drop
        e.drop_cols = drop_cols          # > 0: dropout on the first drop_cols output columns only (mask index n*drop_cols + m)
    if ln_bwd is not None:
        # (x, stats, gamma, partial, dx2 | None, second | None): SMX_EPI_LN_BWD - the GEMM output is the gradient of LN(x)
        x, stats, gamma, partial, dx2, second = ln_bwd[:6]
        if len(ln_bwd) > 6 and ln_bwd[6] is not None:      # (beta, act): the LayerNorm had a fused activation
            e.lnf_beta, e.lnf_act = ln_bwd[6][0].data_ptr(), ln_bwd[6][1]
        e.ln_x, e.ln_ldx = x.data_ptr(), _mat(x)[1]
        if x.dtype == torch.float32 and len(ln_bwd) > 7 and ln_bwd[7]:     # (x float32 next to bf16 gradients)
            e.io_flags |= L.IO_LNX_F32
        e.ln_stats, e.ln_gamma, e.ln_partial = stats.data_ptr(), gamma.data_ptr(), partial.data_ptr()
        e.flags |= L.EPI_LN_BWD
        if dx2 is not None:
            a2, m2, drop2 = second[:3]
            if len(second) > 3 and second[3] is not None:  # (z, act): dx2 = alpha * D(dx * act'(z)) * mask
                assert z is None and act_grad_z is None
                e.z, e.ldz, e.act = second[3].data_ptr(), _mat(second[3])[1], second[4]
            e.ln_dx2, e.ln_lddx2, e.ln_alpha2 = dx2.data_ptr(), _mat(dx2)[1], a2
            e.ln_mask2 = m2.data_ptr() if m2 is not None else None
            if drop2 is not None and drop2[0] > 0.0:
                e.ln_drop_p2, e.ln_drop_seed2 = drop2
    if ln_fwd is not None:
        # (gamma, beta, y, stats | None, eps, act): SMX_EPI_LN_FWD - y = act(LN(output)) appended to the epilogue
        gamma, beta, y, stats, eps, lact = ln_fwd
        e.lnf_gamma, e.lnf_beta = gamma.data_ptr(), beta.data_ptr()
        e.lnf_y, e.lnf_ldy = y.data_ptr(), _mat(y)[1]
        if y.dtype == torch.float32 and out_mode == L.OUT_F32 and res is not None and res.dtype == torch.float32:
            e.io_flags |= L.IO_LNFY_F32                  # the LayerNorm output is the fp32 residual stream itself
        e.lnf_stats = stats.data_ptr() if stats is not None else None
        e.lnf_eps, e.lnf_act = eps, lact
        e.flags |= L.EPI_LN_FWD
    if ln_fwd2 is not None:
        # (gamma2, beta2, y2, stats2 | None, eps2): a SECOND LayerNorm of the first one's output (smx_epilogue.lnf2_*; check
        # smx_gemm_ln_pair_ok first)
        assert ln_fwd is not None
        gamma2, beta2, y2, stats2, eps2 = ln_fwd2
        e.lnf2_gamma, e.lnf2_beta = gamma2.data_ptr(), beta2.data_ptr()
        e.lnf2_y, e.lnf2_ldy = y2.data_ptr(), _mat(y2)[1]
        e.lnf2_stats = stats2.data_ptr() if stats2 is not None else None
        e.lnf2_eps = eps2
    return e


def gemm_symbol(layout, a, b, c, N, M, K, epi=None, batch=1, sa=0, sb=0, sc=0, splits=1, lda=None, ldb=None, ldc=None):
    """The kernel symbol smx_gemm launches for these arguments, spelled as rocprofv3 prints it (smx_gemm_plan_query: the same
    checks and dispatch as the launch itself, nothing launched)."""
    pa, la = _mat(a)
    pb, lb = _mat(b)
    pc, lc = _mat(c)
    plan = L.GemmPlan()
    L.check(L.lib().smx_gemm_plan_query(layout, dt(a), pa, lda or la, sa, pb, ldb or lb, sb, pc, ldc or lc, sc, N, M, K, batch, splits,
                                        ctypes.byref(epi if epi is not None else epilogue()), ctypes.byref(plan)), "smx_gemm_plan_query")
    if plan.kernel == 1:
        return "gemm_tn_dma_kernel"
    if plan.kernel != 0:
        return None
    tb = lambda v: "true" if v else "false"
    return (f"gemm_kernel<{'bf16_t' if a.dtype == torch.bfloat16 else 'float'}, {tb(plan.a_kc)}, {tb(plan.b_kc)}, {plan.tile_n}, "
            f"{plan.tile_m}, {tb(plan.vec)}, {plan.lnf}, {plan.gather}>")


def gemm(layout, a, b, c, N, M, K, epi=None, batch=1, sa=0, sb=0, sc=0, splits=1, lda=None, ldb=None, ldc=None):
    """C (N x M) = epi(op(A) op(B)); a/b/c are 2-D views of batch 0 (batch strides in elements)."""
    pa, la = _mat(a)
    pb, lb = _mat(b)
    pc, lc = _mat(c)
    if epi is None:
        epi = epilogue()
    assert a.dtype == b.dtype
    if epi.colsum:
        epi.workspace = _workspace(L.lib().smx_gemm_colsum_workspace(N, M), c.device, "gemm_colsum").data_ptr()
    tok = None
    if _PROF is not None:
        es, osz = _es(a), (4 if epi.out_mode == L.OUT_F32 else _es(c))
        # algorithmic bytes of the side tensors: residual (float32 on the fp32 residual stream), saved / re-read pre-activation,
        # the LayerNorm input of a fused backward (float32 on the fp32 stream), its second output, the normalised copy of a
        # fused forward (float32 when it is the stream itself)
        side = (4 if epi.io_flags & L.IO_RES_F32 else es) * (1 if epi.res else 0) + es * (1 if epi.z else 0)
        side += (4 if epi.io_flags & L.IO_LNX_F32 else es) * (1 if epi.flags & L.EPI_LN_BWD else 0) + es * (1 if epi.ln_dx2 else 0)
        side += (4 if epi.io_flags & L.IO_LNFY_F32 else es) * (1 if epi.flags & L.EPI_LN_FWD else 0)
        nb = batch * ((N * K + M * K) * es + side * N * M + N * M * osz)
        tag = ("+LNbwd" if epi.flags & L.EPI_LN_BWD else "") + ("+LNfwd" if epi.flags & L.EPI_LN_FWD else "")
        tag += "".join(t for t, on in (("+bias", epi.bias), ("+act", epi.act != L.ACT_NONE and not (epi.flags & L.EPI_ACT_GRAD)),
                                      ("+Z", epi.z and not (epi.flags & L.EPI_ACT_GRAD)), ("+actgrad(z)", epi.flags & L.EPI_ACT_GRAD),
                                      ("+res", epi.res), ("+c0", epi.c0), ("+mask", epi.row_mask), ("+drop", epi.drop_p > 0)) if on)
        tok = _pb(f"gemm {('NT', 'NN', 'TN')[layout]} {'bf16' if es == 2 else 'f32'} ({N}x{K})x({K}x{M}){'' if batch == 1 else ' x%d' % batch} {tag}",
                  nb, 2.0 * N * M * K * batch,
                  gemm_symbol(layout, a, b, c, N, M, K, epi, batch, sa, sb, sc, splits, lda, ldb, ldc))
    L.check(L.lib().smx_gemm(layout, dt(a), pa, lda or la, sa, pb, ldb or lb, sb, pc, ldc or lc, sc, N, M, K, batch,
                             splits, ctypes.byref(epi), _stream()), "smx_gemm")
    _pe(tok)
    return c


def weight_pack(W, transposed=False, bias=None, out=None):
    """MFMA-fragment-order image of a bf16 weight (+ its fp32 bias) for gemm_panel (smx_weight_pack).  W: (M, K) [transposed=False: the
    weight of a forward Linear] or (K, M) [transposed=True: the weight of the Linear whose dgrad dH = dY W is computed]."""
    assert W.dtype == torch.bfloat16 and W.dim() == 2
    M, K = (W.shape[1], W.shape[0]) if transposed else (W.shape[0], W.shape[1])
    if out is None:
        out = torch.empty((L.lib().smx_weight_pack_bytes(M, K) // 2,), dtype=torch.bfloat16, device=W.device)
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == M
    pw, lw = _mat(W)
    tok = _pb(f"weight_pack ({M}x{K}){' T' if transposed else ''}", 4.0 * M * K)
    L.check(L.lib().smx_weight_pack(L.BF16, pw, lw, 1 if transposed else 0, _p(bias), M, K, _p(out), _stream()), "smx_weight_pack")
    _pe(tok)
    return out


def weight_pack_jobs(jobs_dev, njobs, total_blocks, nelem=0):
    """Every job of a device table of smx_pack_job in one launch (smx_weight_pack_jobs)."""
    tok = _pb(f"weight_pack_jobs ({njobs} weights)", 4.0 * nelem)
    L.check(L.lib().smx_weight_pack_jobs(L.BF16, _p(jobs_dev), njobs, total_blocks, _stream()), "smx_weight_pack_jobs")
    _pe(tok)


def gemm_panel_ok(a, M, K):
    return a.dtype == torch.bfloat16 and L.lib().smx_gemm_panel_ok(L.BF16, a.shape[0], M, K) == 1


def gemm_panel(a, wp, c, N, M, K, epi=None):
    """C (N x M) = epi(A Wp) on the panel-resident kernel (smx_gemm_panel): A (N, K) bf16, wp = weight_pack(...)."""
    pa, la = _mat(a)
    pc, lc = _mat(c)
    if epi is None:
        epi = epilogue()
    tok = None
    if _PROF is not None:
        ag = bool(epi.flags & L.EPI_ACT_GRAD)
        nb = (N * K + M * K) * 2 + (2 if epi.z else 0) * N * M + N * M * 2
        tag = "".join(t for t, on in (("+act", epi.act != L.ACT_NONE and not ag), ("+Z", epi.z and not ag),
                                      ("+actgrad(z)", ag), ("+drop", epi.drop_p > 0)) if on)
        tok = _pb(f"gemm panel bf16 ({N}x{K})x({K}x{M}) {tag}", nb, 2.0 * N * M * K,
                  f"gemm_panel_kernel<{K}, {1 if ag else 0}, {epi.act}, {L.lib().smx_gemm_panel_rows(N, M)}>")
    L.check(L.lib().smx_gemm_panel(L.BF16, pa, la, _p(wp), pc, lc, N, M, K, ctypes.byref(epi), _stream()), "smx_gemm_panel")
    _pe(tok)
    return c


def panel_slabs_ok(a, M, K, nslice):
    return a.dtype == torch.bfloat16 and L.lib().smx_gemm_panel_slabs_ok(L.BF16, a.shape[0], M, K, nslice) == 1


def gemm_panel_slabs(a, wp, slabs, N, M, K, nslice):
    """slabs[s] (N x M, fp32) = A[:, s K:(s + 1) K] W_s^T (smx_gemm_panel_slabs): A (N, nslice K) bf16, wp = nslice consecutive
    weight_pack images (weight_pack_slices)."""
    pa, la = _mat(a)
    tok = _pb(f"gemm panel slabs bf16 ({N}x{nslice * K})x({nslice * K}x{M}) S={nslice}", (N * nslice * K + M * nslice * K) * 2 + nslice * N * M * 4,
              2.0 * N * M * K * nslice, f"gemm_panel_kernel<{K}, 2, 0, *>")
    L.check(L.lib().smx_gemm_panel_slabs(L.BF16, pa, la, _p(wp), _p(slabs), N, M, K, nslice, _stream()), "smx_gemm_panel_slabs")
    _pe(tok)
    return slabs


def weight_pack_slices(W, K, transposed=False, out=None):
    """The K-slices of a bf16 weight packed one after the other (no bias) for gemm_panel_slabs.  W (M, nslice K) [transposed=False:
    a forward Linear's weight, slices = column ranges] or (nslice K, M) [transposed=True: the same weight seen from its dgrad,
    slices = row ranges]."""
    Ktot, M = (W.shape[0], W.shape[1]) if transposed else (W.shape[1], W.shape[0])
    ns = Ktot // K
    assert ns * K == Ktot
    per = L.lib().smx_weight_pack_bytes(M, K) // 2
    if out is None:
        out = torch.empty((ns * per,), dtype=torch.bfloat16, device=W.device)
    for s_ in range(ns):
        Ws = W[s_ * K:(s_ + 1) * K] if transposed else W[:, s_ * K:(s_ + 1) * K]
        L.check(L.lib().smx_weight_pack(L.BF16, _p(Ws), Ws.stride(0), 1 if transposed else 0, None, M, K,
                                        ctypes.c_void_p(out.data_ptr() + 2 * s_ * per), _stream()), "smx_weight_pack")
    return out


def slab_epilogue(slabs, nslab, c, N, M, epi):
    """c = epilogue(sum of the float32 slabs) + the LayerNorm(s) the epilogue names (smx_slab_epilogue)."""
    pc, lc = _mat(c)
    tok = _pb(f"slab epilogue ({N}x{M}) S={nslab}{'+LNfwd' if epi.flags & L.EPI_LN_FWD else ''}",
              N * M * (4 * nslab + c.element_size() + (4 if epi.io_flags & L.IO_RES_F32 else 2) * (1 if epi.res else 0) + 2 * (1 if epi.z else 0) +
                       ((4 if epi.io_flags & L.IO_LNFY_F32 else 2) if epi.flags & L.EPI_LN_FWD else 0) + (2 if epi.lnf2_y else 0)))
    L.check(L.lib().smx_slab_epilogue(L.BF16, _p(slabs), nslab, N * M, pc, lc, N, M, ctypes.byref(epi), _stream()), "smx_slab_epilogue")
    _pe(tok)
    return c


def wgrad(dz, x, gW, rows, M, K, batch=1, sz=0, sx=0, sw=0, lddz=None, ldx=None, lddw=None, alpha=1.0, dbias=None):
    """gW[b] (M x K) += alpha * dz[b]^T x[b]  (slab split-K + fixed-order reduction; see smx_linear_wgrad).
    dbias (fp32 (batch, M), contiguous): += alpha * column sums of dz from the same launch (needs K % 4 == 0)."""
    pz, lz = _mat(dz)
    px, lx = _mat(x)
    pw, lw = _mat(gW)
    assert gW.dtype == torch.float32
    if dbias is not None:
        assert dbias.dtype == torch.float32 and dbias.is_contiguous() and dbias.numel() == batch * M and K % 4 == 0
    ws = _workspace(L.lib().smx_linear_wgrad_workspace(rows, M, K, batch), dz.device, slot=1)
    tok = _pb(f"wgrad(+reduce) {'bf16' if _es(dz) == 2 else 'f32'} dW({M}x{K}) over {rows} frames{'' if batch == 1 else ' x%d' % batch}",
              batch * ((M + K) * rows * _es(dz) + 4 * M * K), 2.0 * rows * M * K * batch) if _PROF is not None else None
    L.check(L.lib().smx_linear_wgrad(dt(dz), pz, lddz or lz, sz, px, ldx or lx, sx, pw, lddw or lw, sw, _p(dbias), rows, M, K,
                                     batch, alpha, _p(ws), _stream()), "smx_linear_wgrad")
    _pe(tok)


def wgrad_partial(dz, x, rows, M, K, ws, batch=1, sz=0, sx=0, lddz=None, ldx=None, want_bias=False):
    """Only the split-K slabs of a wgrad (and the bias partials behind them) into the caller-owned workspace `ws`.
    -> (nslabs, slab_stride, bias_offset) in floats; reduce later with reduce_jobs."""
    pz, lz = _mat(dz)
    px, lx = _mat(x)
    n, st, bo = ctypes.c_int32(0), ctypes.c_int64(0), ctypes.c_int64(0)
    tok = _pb(f"wgrad slabs {'bf16' if _es(dz) == 2 else 'f32'} dW({M}x{K}) over {rows} frames{'' if batch == 1 else ' x%d' % batch}",
              batch * ((M + K) * rows * _es(dz) + 4 * M * K), 2.0 * rows * M * K * batch) if _PROF is not None else None
    L.check(L.lib().smx_linear_wgrad_partial(dt(dz), pz, lddz or lz, sz, px, ldx or lx, sx, rows, M, K, batch,
                                             1 if want_bias else 0, _p(ws), ctypes.byref(n), ctypes.byref(st),
                                             ctypes.byref(bo), _stream()), "smx_linear_wgrad_partial")
    _pe(tok)
    return n.value, st.value, bo.value


def wgrad_group(items, nitems, rows, splits):
    """One launch for all the weight gradients of a layer (smx_wgrad_group): `items` is a ctypes array of L.WgradItem with
    workspaces attached; the slabs / bias partials stay in those workspaces for reduce_jobs."""
    tok = None
    if _PROF is not None:
        nb = sum((items[i].M + items[i].K) * rows * 2 + 4 * items[i].M * items[i].K for i in range(nitems))
        fl = sum(2.0 * rows * items[i].M * items[i].K for i in range(nitems))
        tok = _pb(f"wgrad_group bf16 ({nitems} weights: " + " ".join(f"{items[i].M}x{items[i].K}" for i in range(nitems)) +
                  f") over {rows} frames", nb, fl, "wgrad_group_kernel<32>")
    L.check(L.lib().smx_wgrad_group(L.BF16, rows, items, nitems, splits, _stream()), "smx_wgrad_group")
    _pe(tok)


def wgrad_group_direct(recs, rows):
    """All the weight gradients of a layer in one launch, added INTO the gradients (smx_wgrad_group_direct, small batches):
    recs = [(dz, x, gW, dbias | None, M, K), ...] with gW (M, K) float32 views."""
    n = len(recs)
    items = (L.WgradDirectItem * n)()
    for it, (dz, x, gW, dbias, M, K) in zip(items, recs):
        it.dZ, it.lddz, it.X, it.ldx = dz.data_ptr(), dz.stride(0), x.data_ptr(), x.stride(0)
        it.dW, it.lddw, it.dbias, it.M, it.K = gW.data_ptr(), gW.stride(0), (dbias.data_ptr() if dbias is not None else None), M, K
    tok = None
    if _PROF is not None:
        nb = sum((M + K) * rows * 2 + 8 * M * K for _, _, _, _, M, K in recs)
        fl = sum(2.0 * rows * M * K for _, _, _, _, M, K in recs)
        tok = _pb(f"wgrad_group direct bf16 ({n} weights: " + " ".join(f"{M}x{K}" for _, _, _, _, M, K in recs) + f") over {rows} frames", nb, fl,
                  "wgrad_group_direct_kernel")
    L.check(L.lib().smx_wgrad_group_direct(L.BF16, rows, items, n, _stream()), "smx_wgrad_group_direct")
    _pe(tok)


def reduce_jobs(jobs_dev, starts_dev, njobs, total_blocks, nbytes=0):
    tok = _pb(f"reduce_jobs ({njobs} jobs)", nbytes)
    L.check(L.lib().smx_reduce_jobs(_p(jobs_dev), _p(starts_dev), njobs, total_blocks, _stream()), "smx_reduce_jobs")
    _pe(tok)


def act_mask_bwd(dy, z, mask, act, alpha=1.0, dz=None, dbias=None, dgroup=None, gdiv=0, drop=None):
    N, M = dy.shape
    pdy, lddy = _mat(dy)
    pz, ldz = (_mat(z) if z is not None else (None, 0))
    pdz, lddz = (_mat(dz) if dz is not None else (None, 0))
    pg, ldg = (_mat(dgroup) if dgroup is not None else (None, 0))
    ws = _workspace(L.lib().smx_act_mask_bwd_workspace(N, M), dy.device, slot=3) if dbias is not None else None
    dp, ds = (drop if drop is not None else (0.0, 0))
    tok = _pb(f"act_mask_bwd ({N}x{M})", (1 + (z is not None) + (dz is not None)) * N * M * _es(dy))
    L.check(L.lib().smx_act_mask_bwd(dt(dy), pdy, lddy, pz, ldz, _p(mask), pdz, lddz, N, M, act, alpha, _p(dbias), pg,
                                     ldg, gdiv, dp, ds, _epoch(), _p(ws), _stream()), "smx_act_mask_bwd")
    _pe(tok)
    return dz


_ws_cache = {}


def _workspace(nbytes, device, slot=0):
    key = (device, torch.cuda.current_stream().cuda_stream, slot)
    ws = _ws_cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = ws
    return ws


def masked_mean(s, mask, B, T, scale=True, want_inv=False):
    """s: (B*T, D) view; mask: (B*T) uint8 or None -> (out (B,D) fp32, inv_count (B) fp32 | None)."""
    D = s.shape[1]
    ps, lds = _mat(s)
    out = torch.empty((B, D), dtype=torch.float32, device=s.device)
    inv = torch.empty((B,), dtype=torch.float32, device=s.device) if want_inv else None
    ws = _workspace(L.lib().smx_masked_mean_workspace(B, T, D), s.device)
    tok = _pb(f"masked_mean pool ({B},{T},{D})", B * T * D * _es(s) + B * T + 4 * B * D)
    L.check(L.lib().smx_masked_mean_fwd(dt(s), ps, lds, _p(mask), _p(out), _p(inv), B, T, D, 1 if scale else 0, _p(ws),
                                        _stream()), "smx_masked_mean_fwd")
    _pe(tok)
    return out, inv


def bcast_rows(g, inv, ds, B, T, drop=None):
    """ds[b*T+t, :] = D(g[b,:] * inv[b])   (D: optional fused dropout (p, seed), index row * D + col)"""
    pds, ldds = _mat(ds)
    dp, dseed = drop if drop is not None else (0.0, 0)
    tok = _pb(f"bcast_rows ({B},{T},{ds.shape[1]})", B * T * ds.shape[1] * _es(ds))
    L.check(L.lib().smx_masked_mean_bwd(dt(ds), _p(g), _p(inv), pds, ldds, B, T, ds.shape[1], dp, dseed, _epoch(), _stream()),
            "smx_masked_mean_bwd")
    _pe(tok)
    return ds


def pool_bcast_ok(B, T, D):
    return L.lib().smx_pool_bcast_ok(B, T, D) == 1


def pool_bcast(s, mask_in, B, T, ds=None, scale=True, want_mean=True, want_inv=False, inv_in=None, drop=None, z=None, mask_out=None,
               act=L.ACT_NONE):
    """The masked mean over time and its broadcast in ONE launch (smx_pool_bcast; small batches: pool_bcast_ok).
    -> (mean (B, D) fp32 | None, inv_count (B) fp32 | None); ds (B*T, D) receives D(value * inv_in) [* act'(z) * mask_out]."""
    D = s.shape[1]
    ps, lds_ = _mat(s)
    mean = torch.empty((B, D), dtype=torch.float32, device=s.device) if want_mean else None
    inv = torch.empty((B,), dtype=torch.float32, device=s.device) if want_inv else None
    pds, ldds = _mat(ds) if ds is not None else (None, 0)
    pz, ldz = _mat(z) if z is not None else (None, 0)
    dp, dseed = drop if drop is not None else (0.0, 0)
    nb = B * T * D * _es(s) * (1 + (ds is not None) + (z is not None)) + B * T
    tok = _pb(f"pool+bcast ({B},{T},{D})", nb)
    L.check(L.lib().smx_pool_bcast(dt(s), ps, lds_, _p(mask_in), _p(mean), _p(inv_in), _p(inv), pds, ldds, B, T, D, 1 if scale else 0,
                                   dp, dseed, _epoch() if dp > 0 else None, pz, ldz, _p(mask_out), act, _stream()), "smx_pool_bcast")
    _pe(tok)
    return mean, inv


def bcast_rows_act_bwd(g, inv, ds, B, T, z, mask, act):
    """ds[b*T+t, :] = g[b,:] * inv[b] * act'(z[b*T+t, :]) * mask[b*T+t]   (z and / or mask may be None)"""
    pds, ldds = _mat(ds)
    pz, ldz = (_mat(z) if z is not None else (None, 0))
    tok = _pb(f"bcast_rows+act_bwd ({B},{T},{ds.shape[1]})", (1 + (z is not None)) * B * T * ds.shape[1] * _es(ds))
    L.check(L.lib().smx_masked_mean_bwd_act(dt(ds), _p(g), _p(inv), pds, ldds, pz, ldz, _p(mask), act, B, T, ds.shape[1],
                                            _stream()), "smx_masked_mean_bwd_act")
    _pe(tok)
    return ds


def chunk_mean(s, out, B, T, chunk, left, reverse=False):
    D = s.shape[1]
    ps, lds = _mat(s)
    po, ldo = _mat(out)
    ws = _workspace(L.lib().smx_chunk_mean_workspace(B, T, D, chunk), s.device)
    fn = L.lib().smx_chunk_mean_bwd if reverse else L.lib().smx_chunk_mean_fwd
    L.check(fn(dt(s), ps, lds, po, ldo, B, T, D, chunk, -1 if left is None else left, _p(ws), _stream()),
            "smx_chunk_mean")
    return out


def _chunk_summary(name, s, out, B, T, ptrs, dims, left):
    """The launch stream_summary and slot_summary share (smx_<name>; T rows per stream; ptrs / dims: each one's state and sizes)."""
    D = s.shape[1]
    ps, lds = _mat(s)
    po, ldo = _mat(out)
    tok = _pb(f"{name} ({B},{T},{D})", 2 * B * T * D * _es(s))
    L.check(getattr(L.lib(), "smx_" + name)(dt(s), ps, lds, po, ldo, *map(_p, ptrs), B, *dims, D, -1 if left is None else left,
                                            _stream()), "smx_" + name)
    _pe(tok)
    return out


def stream_summary(s, out, B, C_cur, C, left, ring, counter):
    """Streaming DynChunk summary of one chunk (smx_stream_summary): out (B*C_cur, D) rows = the window mean of chunk `counter`;
    the chunk's float32 sums go into `ring` ((B, left, D); (B, D) running sums for left = None; unused for left = 0)."""
    return _chunk_summary("stream_summary", s, out, B, C_cur, (ring, counter), (C_cur, C), left)


def expdecay_mean(s, out, B, T, decay, reverse=False):
    """out = (M s)/rowsum(M) with M_ij = decay^|i-j| (reverse: the transposed operator M (s/rowsum(M))); O(T)."""
    D = s.shape[1]
    ps, lds = _mat(s)
    po, ldo = _mat(out)
    ws = _workspace(L.lib().smx_expdecay_mean_workspace(B, T, D), s.device, slot=5)
    fn = L.lib().smx_expdecay_mean_bwd if reverse else L.lib().smx_expdecay_mean_fwd
    L.check(fn(dt(s), ps, lds, po, ldo, B, T, D, float(decay), _p(ws), _stream()), "smx_expdecay_mean")
    return out


def chunk_mean_sharded(x, out, B, T, D, chunk, left, reverse, c_off, phase, ws, carry=None, carry_c0=0, carry_n=0):
    """One phase of the DynChunk window mean on a sequence-parallel shard (smx_chunk_mean_sharded): phase 1 = chunk sums of x into ws
    ((B, T // chunk, D) float32), phase 2 = window combine (+ carry) into out."""
    px, ldx = _mat(x) if x is not None else (None, 0)
    po, ldo = _mat(out) if out is not None else (None, 0)
    t = x if x is not None else out
    L.check(L.lib().smx_chunk_mean_sharded(dt(t), px, ldx, po, ldo, B, T, D, chunk, -1 if left is None else left, 1 if reverse else 0, c_off,
                                           phase, _p(carry), carry_c0, carry_n, _p(ws), _stream()), "smx_chunk_mean_sharded")


def expdecay_mean_sharded(x, out, B, T, decay, reverse, t_off, T_glob, phase, ends, ws):
    """One phase of the expdecay summary on a sequence-parallel shard (smx_expdecay_mean_sharded): phase 1 fills ends (2, B, D) with the
    states leaving the shard, phase 2 takes the states entering it from `ends` and writes out."""
    D = x.shape[1]
    px, ldx = _mat(x)
    po, ldo = _mat(out) if out is not None else (None, 0)
    L.check(L.lib().smx_expdecay_mean_sharded(dt(x), px, ldx, po, ldo, B, T, D, float(decay), 1 if reverse else 0, t_off, T_glob, phase,
                                              _p(ends), _p(ws), _stream()), "smx_expdecay_mean_sharded")


def layernorm_fwd(x, gamma, beta, eps, want_stats, act=L.ACT_NONE, out_dtype=None, pair=None):
    """y = act(LayerNorm(x)) (smx_layernorm_fwd).  out_dtype (default x.dtype): bf16 output of a float32 input = LayerNorm of the
    fp32 residual stream feeding a bf16 GEMM.  pair = (gamma2, beta2, eps2): the float32 stream x through TWO LayerNorms in one pass
    (the layer-final norm2 + the next layer's first LayerNorm; check layernorm_pair_ok first): y = LN(x) float32, y2 = LN2(y) in
    out_dtype; returns (y, stats, y2, stats2)."""
    N, D = x.shape
    out_dtype = out_dtype or x.dtype
    y = torch.empty((N, D), dtype=torch.float32 if pair is not None else out_dtype, device=x.device)
    stats = torch.empty((N, 2), dtype=torch.float32, device=x.device) if want_stats else None
    a = L.LnFwd(dtype=dt(y), x_f32=int(x.dtype == torch.float32), ldy=D, stats=_p(stats), eps=eps, act=act, N=N, D=D, gamma=_p(gamma),
                beta=_p(beta), Y=_p(y))
    a.X, a.ldx = _mat(x)
    if pair is None:
        assert out_dtype == x.dtype or x.dtype == torch.float32, "mixed LayerNorm: float32 in, compute dtype out"
        tok = _pb(f"layernorm_fwd ({N}x{D})", N * D * (_es(x) + _es(y)))
    else:
        y2 = torch.empty((N, D), dtype=out_dtype, device=x.device)
        st2 = torch.empty((N, 2), dtype=torch.float32, device=x.device) if want_stats else None
        a.gamma2, a.beta2, a.eps2 = _p(pair[0]), _p(pair[1]), pair[2]
        a.Y2, a.ldy2, a.stats2, a.dtype2 = _p(y2), D, _p(st2), dt(y2)
        tok = _pb(f"layernorm_fwd_pair ({N}x{D})", N * D * (4 + 4 + _es(y2)))
    L.check(L.lib().smx_layernorm_fwd(ctypes.byref(a), _stream()), "smx_layernorm_fwd")
    _pe(tok)
    return (y, stats) if pair is None else (y, stats, y2, st2)


def layernorm_pair_ok(x, out_dtype, *affine):
    """Can smx_layernorm_fwd take this float32 stream tensor - and these gamma / beta vectors - in its pair form?  The kernel reads
    all four with 16-byte loads and returns SMX_EUNSUPPORTED for an unaligned one (a parameter that is a view at an odd offset of a
    flat buffer): checked here so that the caller takes the two-launch path instead of failing."""
    return (x.dtype == torch.float32 and x.is_cuda and x.shape[1] % 4 == 0 and x.shape[1] <= 2048 and x.stride(1) == 1
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and out_dtype in (torch.bfloat16, torch.float32)
            and all(v.is_contiguous() and v.data_ptr() % 16 == 0 for v in affine))


def layernorm_fwd_pair(x, gamma1, beta1, eps1, gamma2, beta2, eps2, want_stats, out_dtype):
    """(y1, stats1, y2, stats2): layernorm_fwd's pair form (the layer-final norm2 + the next layer's first LayerNorm)."""
    return layernorm_fwd(x, gamma1, beta1, eps1, want_stats, out_dtype=out_dtype, pair=(gamma2, beta2, eps2))


class Slabs:
    """The float32 split-K partial products of a Linear (gemm_panel_slabs): `t` (S, N, M), to be summed by the consumer -
    slab_epilogue (forward) or layernorm_bwd (the dgrad of the Linear behind a LayerNorm)."""
    def __init__(self, t):
        self.t, self.S, self.N, self.M = t, t.shape[0], t.shape[1], t.shape[2]
        self.shape, self.dtype, self.device = (self.N, self.M), torch.bfloat16, t.device

    def sum(self, dtype=torch.bfloat16):
        """The reduced tensor by plain torch (tests / fallbacks only: the product path fuses the sum into its consumer)."""
        return self.t.sum(0).to(dtype)


def layernorm_bwd(dy, x, gamma, beta, stats, dgamma, dbeta, res=None, act=L.ACT_NONE, ws=None, dx_out=None, second=None, preact=None):
    """dx = res + LayerNorm-backward(dy) (smx_layernorm_bwd).  ws: caller-owned workspace; with dgamma = dbeta = None the partial rows
    stay in it for a deferred reduce_jobs.  dx_out: optional (N, D) destination view (e.g. a column slice of a wider buffer).
    dy: a gradient tensor, or Slabs (the float32 split-K slabs of the dgrad behind the LayerNorm: reducer and LayerNorm backward
    in one launch; dgamma = dbeta = None and ws required).
    second = (alpha, row_mask_u8 | None, (p, seed) | None): also return dx2 = alpha * D(dx) * mask.
    preact = (z, zact): x = zact(z); return the gradient w.r.t. z (check layernorm_bwd_preact_ok first)."""
    N, D = x.shape
    gdt = dy.dtype                                       # gradient dtype; x may be float32 next to bf16 gradients (fp32 residual stream)
    assert x.dtype == gdt or x.dtype == torch.float32
    dx = dx_out if dx_out is not None else torch.empty((N, D), dtype=gdt, device=x.device)
    slabs = isinstance(dy, Slabs)
    if slabs:
        assert dgamma is None and dbeta is None and ws is not None and dy.N == N and dy.M == D
    elif ws is None:
        ws = _workspace(L.lib().smx_layernorm_bwd_workspace(N, D), x.device, slot=2)
    a = L.LnBwd(dtype=L.BF16 if slabs else dt(dy), x_f32=int(x.dtype == torch.float32), act=act, gamma=_p(gamma), beta=_p(beta),
                stats=_p(stats), dX=_p(dx), lddx=_mat(dx)[1], dgamma=_p(dgamma), dbeta=_p(dbeta), workspace=_p(ws), alpha2=1.0,
                epoch=_epoch(), N=N, D=D)
    a.X, a.ldx = _mat(x)
    if slabs:
        a.slabs, a.nslab, a.slab_stride = _p(dy.t), dy.S, N * D
    else:
        a.dY, a.lddy = _mat(dy)
    if res is not None:
        a.R, a.ldr = _mat(res)
    dx2 = None
    if second is not None:
        a2, m2, drop2 = second
        a.alpha2, a.row_mask2 = a2, _p(m2)
        if drop2 is not None and drop2[0] > 0.0:
            a.drop_p2, a.drop_seed2 = drop2
        dx2 = torch.empty((N, D), dtype=gdt, device=x.device)
        a.dX2, a.lddx2 = _p(dx2), D
    if preact is not None:
        a.Z, a.ldz, a.zact = _p(preact[0]), _mat(preact[0])[1], preact[1]
    sfx = f"{'+res' if res is not None else ''}{'+2nd' if second is not None else ''}"
    if slabs:
        tok = _pb(f"layernorm_bwd from slabs ({N}x{D}) S={dy.S}{sfx}", ((1 + (res is not None) + (second is not None)) * 2 + _es(x) + 4 * dy.S) * N * D)
    elif preact is not None:
        tok = _pb(f"layernorm_bwd+preact ({N}x{D})", 4 * _es(dy) * N * D)
    else:
        tok = _pb(f"layernorm_bwd ({N}x{D}){sfx}", ((2 + (res is not None) + (second is not None)) * _es(dy) + _es(x)) * N * D)
    L.check(L.lib().smx_layernorm_bwd(ctypes.byref(a), _stream()), "smx_layernorm_bwd")
    _pe(tok)
    return dx if second is None else (dx, dx2)


def layernorm_bwd_preact_ok(dy, x, z, dx):
    """Can smx_layernorm_bwd take these views in its pre-activation form?  (bf16, D <= 2048, D % 8 == 0, 16-byte aligned rows)"""
    D = x.shape[1]
    ok = lambda t: t.dtype == torch.bfloat16 and t.data_ptr() % 16 == 0 and t.stride(0) % 8 == 0 and t.stride(1) == 1
    return D <= 2048 and D % 8 == 0 and all(ok(t) for t in (dy, x, z, dx))


def layernorm_bwd_preact(dy, x, gamma, beta, stats, z, zact, dgamma, dbeta, act=L.ACT_NONE, ws=None, dx_out=None):
    """dZ = zact'(z) * LayerNorm-backward(dy) for a LayerNorm whose input is x = zact(z): layernorm_bwd's pre-activation form."""
    return layernorm_bwd(dy, x, gamma, beta, stats, dgamma, dbeta, act=act, ws=ws, dx_out=dx_out, preact=(z, zact))


def _dwconv_args(p, w, bias, y, ldy, B, T, D, k, glu, pad_mode, chunk, gate):
    """The smx_dwconv_args both directions share (y: the forward's output or the backward's dY)."""
    a = L.DwconvArgs(dtype=dt(p), glu=1 if glu else 0, w=_p(w), bias=_p(bias), Y=y, ldy=ldy, B=B, T=T, D=D, k=k, pad_mode=pad_mode,
                     chunk=chunk)
    a.P, a.ldp = _mat(p)
    if gate is not None:
        a.gate, a.ldg = _mat(gate)
    return a


def _dwconv_plan(a, backward):
    """smx_dwconv_plan_query: the plan, or None where the library refuses the descriptor."""
    plan = L.DwconvPlan()
    return plan if L.lib().smx_dwconv_plan_query(ctypes.byref(a), backward, ctypes.byref(plan)) == 0 else None


def dwconv_fwd(p, w, bias, B, T, D, k, glu, pad_mode=L.PAD_ZERO, chunk=0, gate=None, drop=None):
    """drop = (p, seed): inverted dropout of the output (the CSGU's own), fused where the kernel can (rolling CSGU path),
    else a separate in-place smx_dropout with the same mask."""
    y = torch.empty((B * T, D), dtype=p.dtype, device=p.device)
    a = _dwconv_args(p, w, bias, _p(y), D, B, T, D, k, glu, pad_mode, chunk, gate)
    tok = _pb(f"dwconv_fwd ({B},{T},{D}) k={k}", 3 * B * T * D * _es(p))
    fused = False
    if drop is not None and drop[0] > 0.0 and _CSGU_DROP_FUSE:
        a.drop_p, a.drop_seed, a.epoch = drop[0], drop[1], _epoch()
        fused = _dwconv_plan(a, 0) is not None                     # (refused: the separate pass below)
        a.drop_p = drop[0] if fused else 0.0
    L.check(L.lib().smx_dwconv_fwd(ctypes.byref(a), _stream()), "smx_dwconv_fwd")
    _pe(tok)
    if drop is not None and drop[0] > 0.0 and not fused:
        dropout(y, drop[0], drop[1], out=y)
    return y


def _chunk_dwconv(kind, p, w, bias, state, slots, B, T, D, k):
    """The launch dwconv_stream and dwconv_slots share (smx_dwconv1d_glu_<kind>; T rows per stream; slots: () | (valid, counters))."""
    assert state.dtype == p.dtype and state.is_contiguous() and state.shape == (B, (k - 1) // 2, 2 * D)
    y = torch.empty((B * T, D), dtype=p.dtype, device=p.device)
    pp, ldp = _mat(p)
    tok = _pb(f"dwconv_{kind} ({B},{T},{D}) k={k}", 3 * B * T * D * _es(p))
    L.check(getattr(L.lib(), "smx_dwconv1d_glu_" + kind)(dt(p), pp, ldp, _p(w), _p(bias), _p(state), _p(y), D, *map(_p, slots), B, T, D,
                                                         k, _stream()), "smx_dwconv1d_glu_" + kind)
    _pe(tok)
    return y


def dwconv_stream(p, w, bias, state, B, C_cur, D, k):
    """GLU + depthwise conv over one chunk of B streams (smx_dwconv1d_glu_stream): rows before the chunk come from `state`
    ((B, (k-1)/2, 2D), compute dtype), which the kernel then replaces in place with the chunk's last (k-1)/2 pre-GLU rows."""
    return _chunk_dwconv("stream", p, w, bias, state, (), B, C_cur, D, k)


def stream_advance(counter, table, pe, C):
    """End of a chunk step (smx_stream_advance): counter += 1 and pe (C, D) = the table's rows of the next chunk."""
    assert table.dtype == pe.dtype
    pt, ldt = _mat(table)
    pp, ldpe = _mat(pe)
    L.check(L.lib().smx_stream_advance(dt(pe), _p(counter), pt, ldt, table.shape[0], pp, ldpe, C, pe.shape[1], _stream()),
            "smx_stream_advance")


def slot_summary(s, out, B, C, left, ring, counters, valid):
    """Per-slot streaming DynChunk summary (smx_slot_summary): s / out (B*C, D), slot b's rows b*C .. b*C + valid[b] - 1 = the window
    mean of its chunk counters[b]; `valid` (B,) int32 and `counters` (B,) int64 on the device.  Slots with valid 0 are untouched."""
    return _chunk_summary("slot_summary", s, out, B, C, (ring, counters, valid), (C,), left)


def dwconv_slots(p, w, bias, state, valid, counters, B, C, D, k):
    """GLU + depthwise conv of one slot step (smx_dwconv1d_glu_slots): dwconv_stream per slot with C_cur = valid[b]; the state reads
    as zero where counters[b] == 0 and is left untouched where valid[b] == 0."""
    return _chunk_dwconv("slots", p, w, bias, state, (valid, counters), B, C, D, k)


def slot_begin(counters, start, table, pe, B, C, D):
    """First launch of a slot step (smx_slot_begin): counters[b] = 0 where start[b], then pe (B*C, D) = each slot's rows of the
    positional table (table / pe None: counters only)."""
    if pe is None:
        pt, ldt, rows, pp, ldpe, code = None, D, 0, None, D, L.F32
    else:
        assert table.dtype == pe.dtype
        (pt, ldt), (pp, ldpe), rows, code = _mat(table), _mat(pe), table.shape[0], dt(pe)
    L.check(L.lib().smx_slot_begin(code, _p(counters), _p(start), pt, ldt, rows, pp, ldpe, B, C, D, _stream()), "smx_slot_begin")


def slot_advance(counters, valid, B, C):
    """Last launch of a slot step (smx_slot_advance): counters[b] += (valid[b] == C)."""
    L.check(L.lib().smx_slot_advance(_p(counters), _p(valid), B, C, _stream()), "smx_slot_advance")


def dwconv_bwd(dy, p, w, bias, dw, dbias, B, T, D, k, glu, pad_mode=L.PAD_ZERO, chunk=0, gate=None, dgate_out=None, ws=None):
    """ws (caller-owned, smx_dwconv1d_glu_bwd_workspace bytes): the tap / bias partial rows stay in it for a deferred
    reduce_jobs and dw / dbias are not touched; then returns (dp, dgate, rows) - the number of partial rows left in ws
    (smx_dwconv_plan.partial_rows), or 0 where the plan is not deferrable and the gradients went into dw / dbias directly."""
    dp = torch.empty((B * T, p.shape[1]), dtype=p.dtype, device=p.device)
    dgate = None
    if gate is not None:
        dgate = dgate_out if dgate_out is not None else torch.empty((B * T, D), dtype=p.dtype, device=p.device)
    a = _dwconv_args(p, w, bias, *_mat(dy), B, T, D, k, glu, pad_mode, chunk, gate)
    a.dP, a.lddp, a.dw, a.dbias, a.workspace = _p(dp), dp.shape[1], _p(dw), _p(dbias), _p(ws)
    if dgate is not None:
        a.dgate, a.lddg = _mat(dgate)
    tok = _pb(f"dwconv_bwd ({B},{T},{D}) k={k}", 5 * B * T * D * _es(p))
    plan = _dwconv_plan(a, 1) if ws is not None else None
    rows = plan.partial_rows if plan is not None and plan.deferrable else 0
    if rows:
        a.dw = a.dbias = None
    else:
        a.workspace = _p(_workspace(L.lib().smx_dwconv1d_glu_bwd_workspace(B, T, D, k), p.device, slot=4))
    L.check(L.lib().smx_dwconv_bwd(ctypes.byref(a), _stream()), "smx_dwconv_bwd")
    _pe(tok)
    return (dp, dgate, rows) if ws is not None else (dp, dgate)


def axpby(a, x, b=0.0, y0=None, out=None):
    N, D = x.shape
    if out is None:
        out = torch.empty((N, D), dtype=x.dtype, device=x.device)
    px, ldx = _mat(x)
    py0, ldy0 = (_mat(y0) if y0 is not None else (None, 0))
    po, ldo = _mat(out)
    L.check(L.lib().smx_axpby(dt(x), a, px, ldx, b, py0, ldy0, po, ldo, N, D, _stream()), "smx_axpby")
    return out


_drop_state = {"counter": 0}


def new_dropout_seed():
    """A fresh 64-bit seed per dropout site and call, derived from torch's global seed and a call counter (no
    device sync)."""
    _drop_state["counter"] += 1
    # salt: 0, or rank + 1 of a sequence-parallel shard (set_seed_salt) - the fused masks are indexed by the LOCAL frame row, so every
    # shard must draw from a seed of its own; forward and backward of a site use the same returned value either way
    return (torch.initial_seed() * 0x9E3779B97F4A7C15 + _drop_state["counter"] * 0xD1B54A32D192ED03 +
            _drop_state.get("salt", 0) * 0xA24BAED4963EE407) & 0xFFFFFFFFFFFFFFFF


def set_seed_salt(salt):
    """Per-process salt of every dropout seed drawn from now on (sequence_parallel: rank + 1 inside the context, 0 outside)."""
    prev = _drop_state.get("salt", 0)
    _drop_state["salt"] = int(salt)
    return prev


def dropout(x, p, seed, out=None):
    """out = dropout(x) with the counter-based mask of `seed` (call again on the gradient for the backward)."""
    N, D = x.shape
    if out is None:
        out = torch.empty((N, D), dtype=x.dtype, device=x.device)
    px, ldx = _mat(x)
    po, ldo = _mat(out)
    tok = _pb(f"dropout ({N}x{D})", 2 * N * D * _es(x))
    L.check(L.lib().smx_dropout(dt(x), px, ldx, po, ldo, N, D, p, seed, _epoch(), _stream()), "smx_dropout")
    _pe(tok)
    return out


def add_rowtable(y, table, R):
    N, D = y.shape
    py, ldy = _mat(y)
    L.check(L.lib().smx_add_rowtable(dt(y), py, ldy, _p(table), R, N, D, _stream()), "smx_add_rowtable")
    return y


def cast(src, dtype):
    """fp32 <-> compute dtype through the library's cast kernels (contiguous tensors)."""
    if src.dtype == dtype:
        return src
    src = src.contiguous()
    dst = torch.empty(src.shape, dtype=dtype, device=src.device)
    if src.dtype == torch.float32:
        L.check(L.lib().smx_cast_from_f32(_DT[dtype], _p(src), _p(dst), src.numel(), _stream()), "smx_cast_from_f32")
    elif dtype == torch.float32:
        L.check(L.lib().smx_cast_to_f32(_DT[src.dtype], _p(src), _p(dst), src.numel(), _stream()), "smx_cast_to_f32")
    else:
        return cast(cast(src, torch.float32), dtype)
    return dst


def adamw_step(param, grad, m, v, shadow, lr, b1, b2, eps, wd, step, grad_scale=1.0, gscale_dev=None, lr_dev=None):
    tok = _pb(f"adamw ({param.numel()} params)", (28 + (2 if shadow is not None else 0)) * param.numel())
    if lr_dev is None:
        L.check(L.lib().smx_adamw_step(_p(param), _p(grad), _p(m), _p(v), _p(shadow), param.numel(), lr, b1, b2, eps, wd,
                                       step, grad_scale, _p(gscale_dev), _epoch() if step <= 0 else None, _stream()), "smx_adamw_step")
    else:                             # the rate of this update is in device memory (lr_schedule below)
        L.check(L.lib().smx_adamw_step_lr(_p(param), _p(grad), _p(m), _p(v), _p(shadow), param.numel(), lr, _p(lr_dev), b1, b2,
                                          eps, wd, step, grad_scale, _p(gscale_dev), _epoch() if step <= 0 else None, _stream()),
                "smx_adamw_step_lr")
    _pe(tok)


SGD_GRID_SWEEP = L.SGD_MAX_BLOCKS * 256 * 4     # elements one sweep of smx_sgd_step's capped grid covers


def sgd_step(param, grad, buf, shadow, lr, momentum=0.0, wd=0.0, nesterov=False, grad_scale=1.0, gscale_dev=None, lr_dev=None):
    """torch.optim.SGD (dampening 0) on a flat fp32 range, in place; buf: the momentum buffer (None with momentum 0)."""
    n = param.numel()
    tok = _pb(f"sgd ({n} params)", (12 + (8 if buf is not None else 0) + (2 if shadow is not None else 0)) * n)
    L.check(L.lib().smx_sgd_step(_p(param), _p(grad), _p(buf), _p(shadow), n, lr, _p(lr_dev), momentum, wd, int(bool(nesterov)),
                                 grad_scale, _p(gscale_dev), _stream()), "smx_sgd_step")
    _pe(tok)


def lr_schedule(kind, consts, lr0, step, out):
    """out[0] (device float32) = the rate of update `step` (> 0: by value; <= 0: read from the device step counter of
    set_step_counter) under schedule `kind` (L.LR_NOAM / L.LR_WARM_EXP_DECAY) with its four constants (include/smx.h)."""
    assert out.is_cuda and out.dtype == torch.float32
    c = [float(x) for x in consts] + [0.0] * (4 - len(consts))
    L.check(L.lib().smx_lr_schedule(kind, c[0], c[1], c[2], c[3], float(lr0), int(step), _epoch() if step <= 0 else None,
                                    _p(out), _stream()), "smx_lr_schedule")


def utt_meanstd(x2, lens, mean, std, B, T, mean_norm=True, std_norm=True, eps=1e-10):
    px, ldx = _mat(x2)
    L.check(L.lib().smx_utt_meanstd(dt(x2), px, ldx, _p(lens), _p(mean), _p(std), B, T, x2.shape[1], int(mean_norm),
                                    int(std_norm), eps, _stream()), "smx_utt_meanstd")


def stats_combine(cur_mean, cur_std, glob_mean, glob_std, weight):
    B, F = cur_mean.shape
    L.check(L.lib().smx_stats_combine(_p(cur_mean), _p(cur_std), B, F, _p(glob_mean), _p(glob_std), float(weight), _stream()),
            "smx_stats_combine")


def colnorm(x2, mean, std, stat_stride, out, B, T):
    px, ldx = _mat(x2)
    po, ldo = _mat(out)
    L.check(L.lib().smx_colnorm(dt(x2), px, ldx, _p(mean), _p(std), stat_stride, po, ldo, B, T, x2.shape[1], _stream()),
            "smx_colnorm")


SPECAUG_HDR = 8     # header words of the spec-augment parameter block (include/smx.h)


def specaug_params_words(B, n_time_cap, n_freq_cap):
    """int32 words of the parameter block of smx_specaug_draw / smx_specaug_apply."""
    nbytes = L.lib().smx_specaug_params_bytes(B, n_time_cap, n_freq_cap)
    if nbytes == 0:
        raise ValueError(f"spec-augment block: B = {B} must be positive and the caps ({n_time_cap}, {n_freq_cap}) within 0 .. 32")
    return nbytes // 4


def specaug_draw(params, B, T, F, stages, time_drop, freq_drop, window, seed):
    """Fill `params` on the device.  time_drop / freq_drop: (len_lo, len_hi, cnt_lo, cnt_hi) or None; the step counter is mixed in."""
    assert params.is_cuda, NO_CPU
    t, f = time_drop or (0, 1, 0, 0), freq_drop or (0, 1, 0, 0)
    ntc, nfc = (t[3] if stages & L.SPECAUG_TIME else 0), (f[3] if stages & L.SPECAUG_FREQ else 0)
    assert params.dtype == torch.int32 and params.is_contiguous() and params.numel() >= specaug_params_words(B, ntc, nfc)
    L.check(L.lib().smx_specaug_draw(_p(params), B, T, F, stages, t[0], t[1], t[2], t[3], f[0], f[1], f[2], f[3], window,
                                     seed & 0xFFFFFFFFFFFFFFFF, _epoch(), _stream()), "smx_specaug_draw")
    return params


def specaug_apply(x, params, n_time_cap, n_freq_cap, out=None):
    """x (B, T, F) -> the augmented copy: one pass over x with the draws of `params` (smx_specaug_apply)."""
    if not x.is_cuda or not params.is_cuda:
        raise RuntimeError(NO_CPU)
    B, T, F = x.shape
    assert params.dtype == torch.int32 and params.is_contiguous() and params.numel() >= specaug_params_words(B, n_time_cap, n_freq_cap)
    x2 = rows2d(x)
    if out is None:
        out = torch.empty((B, T, F), dtype=x.dtype, device=x.device)
    o2 = rows2d(out)
    assert o2.data_ptr() == out.data_ptr() and o2.dtype == x.dtype
    px, ldx = _mat(x2)
    po, ldo = _mat(o2)
    tok = _pb(f"specaug ({B}x{T}x{F})", 2 * B * T * F * _es(x))
    L.check(L.lib().smx_specaug_apply(dt(x), px, ldx, po, ldo, _p(params), B, T, F, n_time_cap, n_freq_cap, _stream()),
            "smx_specaug_apply")
    _pe(tok)
    return out


class ResamplePlan(collections.namedtuple("ResamplePlan", "o n width K taps tile_blocks image")):
    """smx_resample_plan's result: the reduced rates, the filter's half width and length, the longest run of nonzero taps, the
    n-sample output blocks per workgroup tile, and the plan image (int32 words, on the CPU) of include/smx.h."""
    __slots__ = ()

    def out_len(self, L):
        """ceil(n L / o) in exact integers."""
        return (self.n * int(L) + self.o - 1) // self.o

    def first(self):
        return self.image[8:8 + self.n]

    def weights(self):
        return self.image[8 + self.n:].view(torch.float32).view(self.n, self.taps)


def resample_plan(orig_freq, new_freq):
    """The polyphase plan of orig_freq -> new_freq (host arithmetic, no GPU).  NotImplementedError for a ratio the kernel cannot
    hold (SMX_EUNSUPPORTED: the table or one block's input does not fit LDS, a rate <= 0)."""
    info = (ctypes.c_int32 * 8)()
    nbytes = ctypes.c_size_t(0)
    code = L.lib().smx_resample_plan(int(orig_freq), int(new_freq), info, ctypes.byref(nbytes), None, 0)
    if code == -2:
        raise NotImplementedError(L.lib().smx_last_error().decode())
    L.check(code, "smx_resample_plan")
    image = torch.zeros(nbytes.value // 4, dtype=torch.int32)
    L.check(L.lib().smx_resample_plan(int(orig_freq), int(new_freq), info, None, ctypes.c_void_p(image.data_ptr()), nbytes.value),
            "smx_resample_plan")
    return ResamplePlan(*list(info)[:6], image)


def resample(x2, image, out2, L_in):
    """out2[b][0, L_out) = the resampled x2[b][0, L_in): x2 (B, >= L_in), out2 (B, L_out) float32 views with unit inner stride, image
    the plan image on their device (smx_resample).  L_out is out2's width and the caller's to get right (ResamplePlan.out_len)."""
    if not (x2.is_cuda and out2.is_cuda and image.is_cuda):
        raise RuntimeError(NO_CPU)
    assert x2.dtype == torch.float32 and out2.dtype == torch.float32 and image.dtype == torch.int32 and image.is_contiguous()
    B = x2.shape[0]
    assert out2.shape[0] == B and x2.shape[1] >= L_in
    px, ldx = _mat(x2)
    po, ldo = _mat(out2)
    tok = _pb(f"resample ({B}x{L_in})", 4 * B * (L_in + out2.shape[1]))
    L.check(L.lib().smx_resample(px, ldx, po, ldo, _p(image), B, L_in, _stream()), "smx_resample")
    _pe(tok)
    return out2


def log_softmax_fwd(x, out=None):
    """log_softmax over the last dim of a (N, V) view (out: a contiguous (N, V) buffer of x's dtype to write instead of a fresh one)."""
    N, V = x.shape
    y = torch.empty((N, V), dtype=x.dtype, device=x.device) if out is None else out
    assert y.is_cuda and y.is_contiguous() and y.dtype == x.dtype and tuple(y.shape) == (N, V)
    px, ldx = _mat(x)
    L.check(L.lib().smx_log_softmax_fwd(dt(x), px, ldx, _p(y), V, N, V, _stream()), "smx_log_softmax_fwd")
    return y


def log_softmax_bwd(dy, y):
    N, V = y.shape
    dx = torch.empty((N, V), dtype=y.dtype, device=y.device)
    pdy, lddy = _mat(dy)
    py, ldy = _mat(y)
    L.check(L.lib().smx_log_softmax_bwd(dt(y), pdy, lddy, py, ldy, _p(dx), V, N, V, _stream()), "smx_log_softmax_bwd")
    return dx


def ctc_fwd(lp2, targets, in_len, tgt_len, B, T, blank):
    """lp2: (B*T, V) log-probabilities; targets int32 (B, Smax); lengths int32 (B).  -> (nll (B) fp32, workspace)."""
    V, Smax = lp2.shape[1], targets.shape[1]
    assert targets.dtype == torch.int32 and in_len.dtype == torch.int32 and tgt_len.dtype == torch.int32
    assert targets.is_contiguous()
    nll = torch.empty((B,), dtype=torch.float32, device=lp2.device)
    ws = torch.empty(max(L.lib().smx_ctc_workspace(B, T, Smax), 16), dtype=torch.uint8, device=lp2.device)  # kept for the bwd
    plp, ldlp = _mat(lp2)
    L.check(L.lib().smx_ctc_loss_fwd(dt(lp2), plp, ldlp, _p(targets), _p(in_len), _p(tgt_len), B, T, V, Smax, blank, _p(nll),
                                     _p(ws), _stream()), "smx_ctc_loss_fwd")
    return nll, ws


def ctc_bwd(lp2, targets, in_len, tgt_len, B, T, blank, nll, gscale, ws):
    V, Smax = lp2.shape[1], targets.shape[1]
    g = torch.empty((B * T, V), dtype=lp2.dtype, device=lp2.device)
    plp, ldlp = _mat(lp2)
    L.check(L.lib().smx_ctc_loss_bwd(dt(lp2), plp, ldlp, _p(targets), _p(in_len), _p(tgt_len), B, T, V, Smax, blank, _p(nll),
                                     _p(gscale), _p(g), V, _p(ws), _stream()), "smx_ctc_loss_bwd")
    return g


# ---- label-smoothed sequence losses + accuracy (csrc/seqloss.hip).  x (B, U, V) with unit stride along V and any row / batch strides
# (a truncated view is not copied); targets int32 (B, >= U) with unit stride along U; keep_len int32 (B) on the device or None.
def _seq3(x, targets, keep_len):
    if not (x.is_cuda and targets.is_cuda and (keep_len is None or keep_len.is_cuda)):
        raise RuntimeError(NO_CPU)
    assert x.dim() == 3 and targets.dim() == 2 and targets.dtype == torch.int32
    B, U, V = x.shape
    assert targets.shape[0] == B and targets.shape[1] >= U and (targets.shape[1] <= 1 or targets.stride(1) == 1)
    assert V == 1 or x.stride(2) == 1, f"need unit stride along the vocabulary, got {x.stride()}"
    assert keep_len is None or (keep_len.dtype == torch.int32 and keep_len.shape == (B,) and keep_len.is_contiguous())
    ldx = x.stride(1) if U > 1 else max(x.stride(1), V)
    bsx = x.stride(0) if B > 1 else 0
    ldt = targets.stride(0) if B > 1 else max(targets.stride(0), U)
    return B, U, V, ldx, bsx, ldt


def seqloss_fwd(x, targets, keep_len, pad_idx, conf, off, cst, from_logits, want_hits=True):
    """-> (row_loss (B, U) fp32, lse (B, U, 2) fp32 or None, row_flags (B, U) int32, utt_loss (B) fp32, utt_kept (B) int32,
    utt_hits (B) int32 or None): smx_seqloss_fwd.  No host synchronisation."""
    B, U, V, ldx, bsx, ldt = _seq3(x, targets, keep_len)
    dev = x.device
    row_loss = torch.empty((B, U), dtype=torch.float32, device=dev)
    flags = torch.empty((B, U), dtype=torch.int32, device=dev)
    lse = torch.empty((B, U, 2), dtype=torch.float32, device=dev) if from_logits else None
    utt_loss = torch.empty((B,), dtype=torch.float32, device=dev)
    utt_kept = torch.empty((B,), dtype=torch.int32, device=dev)
    utt_hits = torch.empty((B,), dtype=torch.int32, device=dev) if want_hits else None
    tok = _pb(f"seqloss_fwd {'logits' if from_logits else 'logprobs'} {'bf16' if _es(x) == 2 else 'f32'} ({B},{U},{V})",
              B * U * V * _es(x) + B * U * (8 + 4 + (8 if from_logits else 0)))
    L.check(L.lib().smx_seqloss_fwd(dt(x), int(bool(from_logits)), _p(x), ldx, bsx, _p(targets), ldt, _p(keep_len), B, U, V, int(pad_idx),
                                    float(conf), float(off), float(cst), _p(row_loss), _p(lse), _p(flags), _p(utt_loss), _p(utt_kept),
                                    _p(utt_hits), _stream()), "smx_seqloss_fwd")
    _pe(tok)
    return row_loss, lse, flags, utt_loss, utt_kept, utt_hits


def seqloss_bwd(x, targets, keep_len, pad_idx, conf, off, lse, g, from_logits, out=None):
    """g (B, U) fp32 contiguous -> dX (B, U, V) in x's dtype (torch.empty: the kernel writes every element, zeros for dropped rows):
    smx_seqloss_bwd."""
    B, U, V, ldx, bsx, ldt = _seq3(x, targets, keep_len)
    assert g.is_cuda and g.dtype == torch.float32 and g.shape == (B, U) and g.is_contiguous()
    assert not from_logits or (lse is not None and lse.shape == (B, U, 2) and lse.is_contiguous())
    if out is None:
        out = torch.empty((B, U, V), dtype=x.dtype, device=x.device)
    assert out.shape == (B, U, V) and out.dtype == x.dtype and out.is_contiguous()
    tok = _pb(f"seqloss_bwd {'logits' if from_logits else 'logprobs'} {'bf16' if _es(x) == 2 else 'f32'} ({B},{U},{V})",
              (2 if from_logits else 1) * B * U * V * _es(x) + B * U * (8 + (8 if from_logits else 0)))
    L.check(L.lib().smx_seqloss_bwd(dt(x), int(bool(from_logits)), _p(x) if from_logits else None, ldx, bsx, _p(targets), ldt,
                                    _p(keep_len), B, U, V, int(pad_idx), float(conf), float(off), _p(lse), _p(g), _p(out), V, _stream()),
            "smx_seqloss_bwd")
    _pe(tok)
    return out


# ---- transducer head (csrc/transducer.hip).  Lattice rows (b, t, u), u fastest; every size below comes from tensor shapes and the
# lengths stay on the device: no call here synchronises with the host.
def transducer_joint_fwd(enc, dec, act):
    """enc (B, T, J), dec (B, U1, J) contiguous, same dtype -> H (B, T, U1, J)."""
    B, T, J = enc.shape
    U1 = dec.shape[1]
    H = torch.empty((B, T, U1, J), dtype=enc.dtype, device=enc.device)
    L.check(L.lib().smx_transducer_joint_fwd(dt(enc), _p(enc), _p(dec), _p(H), B, T, U1, J, act, _stream()), "smx_transducer_joint_fwd")
    return H


def transducer_joint_bwd(dH, enc, dec, act, d_enc=None, d_dec=None):
    """dH (B, T, U1, J) -> (d_enc (B, T, J), d_dec (B, U1, J)), written into d_enc / d_dec when given (contiguous views)."""
    B, T, J = enc.shape
    U1 = dec.shape[1]
    d_enc = torch.empty_like(enc) if d_enc is None else d_enc
    d_dec = torch.empty_like(dec) if d_dec is None else d_dec
    ws = _workspace(L.lib().smx_transducer_joint_bwd_workspace(B, T, U1, J), enc.device, "transducer_joint")
    L.check(L.lib().smx_transducer_joint_bwd(dt(enc), _p(dH), _p(enc), _p(dec), _p(d_enc), _p(d_dec), B, T, U1, J, act, _p(ws),
                                             _stream()), "smx_transducer_joint_bwd")
    return d_enc, d_dec


def _row_f32(rows, device, n):
    return [torch.empty((rows,), dtype=torch.float32, device=device) for _ in range(n)]


def transducer_row_stats(z2, targets, B, T, U1, blank):
    """z2 (B T U1, V) logits -> (lse, lp_blank, lp_y), fp32 per lattice row."""
    V = z2.shape[1]
    lse, lpb, lpy = _row_f32(z2.shape[0], z2.device, 3)
    pz, ldz = _mat(z2)
    L.check(L.lib().smx_transducer_row_stats(dt(z2), pz, ldz, _p(targets), B, T, U1, V, blank, _p(lse), _p(lpb), _p(lpy), _stream()),
            "smx_transducer_row_stats")
    return lse, lpb, lpy


def transducer_loss_fwd(lpb, lpy, in_len, tgt_len, B, T, U1):
    """-> (nll (B) fp32, alpha (B T U1 + B) fp64 kept for the backward: the forward variables, then -log P)."""
    alpha = torch.empty((lpb.numel() + B,), dtype=torch.float64, device=lpb.device)
    nll = torch.empty((B,), dtype=torch.float32, device=lpb.device)
    L.check(L.lib().smx_transducer_loss_fwd(_p(lpb), _p(lpy), _p(in_len), _p(tgt_len), B, T, U1, _p(alpha), _p(nll), _stream()),
            "smx_transducer_loss_fwd")
    return nll, alpha


def transducer_loss_bwd(lpb, lpy, alpha, gscale, in_len, tgt_len, B, T, U1):
    """-> (g_blank, g_y) per lattice row, fp32, already scaled by gscale[b]."""
    gb, gy = torch.empty_like(lpb), torch.empty_like(lpb)
    L.check(L.lib().smx_transducer_loss_bwd(_p(lpb), _p(lpy), _p(alpha), _p(gscale), _p(in_len), _p(tgt_len), B, T, U1,
                                            _p(gb), _p(gy), _stream()), "smx_transducer_loss_bwd")
    return gb, gy


def transducer_logit_grad(z2, targets, lse, gb, gy, B, T, U1, blank):
    V = z2.shape[1]
    dz = torch.empty((z2.shape[0], V), dtype=z2.dtype, device=z2.device)
    pz, ldz = _mat(z2)
    L.check(L.lib().smx_transducer_logit_grad(dt(z2), pz, ldz, _p(targets), _p(lse), _p(gb), _p(gy), B, T, U1, V, blank, _p(dz), V,
                                              _stream()), "smx_transducer_logit_grad")
    return dz


def transducer_fused_ok(dtype, J, V):
    return bool(L.lib().smx_transducer_fused_ok(_DT[dtype], J, V))


def transducer_gemm_stats(H2, W, bias, targets, B, T, U1, blank):
    """H2 (B T U1, J), W (V, J) same dtype, bias fp32 (V) or None -> (lse, lp_blank, lp_y); the logits are never stored."""
    rows, J = H2.shape
    V = W.shape[0]
    lse, lpb, lpy = _row_f32(rows, H2.device, 3)
    ws = torch.empty(L.lib().smx_transducer_stats_workspace(rows, V), dtype=torch.uint8, device=H2.device)
    tok = _pb(f"transducer_gemm_stats {'bf16' if H2.dtype == torch.bfloat16 else 'f32'} ({rows}x{J})x({J}x{V})",
              (rows * J + V * J) * _es(H2) + rows * 12, 2.0 * rows * J * V)
    L.check(L.lib().smx_transducer_gemm_stats(dt(H2), _p(H2), _p(W), _p(bias), _p(targets), B, T, U1, J, V, blank, _p(lse), _p(lpb),
                                              _p(lpy), _p(ws), _stream()), "smx_transducer_gemm_stats")
    _pe(tok)
    return lse, lpb, lpy


def transducer_gemm_grad(H2, W, bias, targets, lse, gb, gy, B, T, U1, blank, row0, nrows, dz):
    """dz (nrows, V) view (unit column stride, any 16-byte multiple leading dimension) = the logit gradient of lattice rows
    [row0, row0 + nrows), the logits recomputed tile by tile."""
    J = H2.shape[1]
    V = W.shape[0]
    pdz, lddz = _mat(dz)
    tok = _pb(f"transducer_gemm_grad {'bf16' if H2.dtype == torch.bfloat16 else 'f32'} ({nrows}x{J})x({J}x{V})",
              (nrows * J + V * J + nrows * V) * _es(H2) + nrows * 12, 2.0 * nrows * J * V)
    L.check(L.lib().smx_transducer_gemm_grad(dt(H2), _p(H2), _p(W), _p(bias), _p(targets), _p(lse), _p(gb), _p(gy), B, T, U1, J, V,
                                             blank, row0, nrows, pdz, lddz, _stream()), "smx_transducer_gemm_grad")
    _pe(tok)
    return dz


# ---- prediction network (csrc/lstm.hip): one-hot Embedding rows, the one-hot input route of the LSTM, the recurrence and its BPTT.
def _tokens_i32(tokens):
    assert tokens.is_cuda, NO_CPU
    return tokens.reshape(-1).to(torch.int32).contiguous()


def lstm_ok(dtype, H):
    return bool(L.lib().smx_lstm_ok(_DT[dtype], H))


def onehot_rows(tokens, V, blank, dtype):
    """tokens (...) integer -> (..., V - 1) one-hot rows without the blank's column (the blank: a zero row)."""
    tk = _tokens_i32(tokens)
    Y = torch.empty((tk.numel(), V - 1), dtype=dtype, device=tk.device)
    L.check(L.lib().smx_onehot_rows(_DT[dtype], _p(tk), _p(Y), V - 1, tk.numel(), V, blank, _stream()), "smx_onehot_rows")
    return Y.view(*tokens.shape, V - 1)


def token_keep(n, p, seed, device):
    """The n per-token factors (0 or 1 / (1 - p), fp32) of the prediction network's embedding dropout for `seed`: smx_dropout on a
    column of ones, so mask index = token index (and the device step counter applies as to every dropout)."""
    return dropout(torch.ones((n, 1), dtype=torch.float32, device=device), p, seed).view(n)


def onehot_gates_fwd(tk32, keep, WihT, bias, V, blank):
    """tk32 (rows) int32, WihT (V - 1, G) = W_ih^T, bias (G) fp32, keep (rows) fp32 or None -> Gx (rows, G) fp32."""
    rows, G = tk32.numel(), WihT.shape[1]
    Gx = torch.empty((rows, G), dtype=torch.float32, device=tk32.device)
    pw, ldw = _mat(WihT)
    tok = _pb(f"onehot_gates_fwd ({rows}x{G})", rows * G * (4 + _es(WihT)))
    L.check(L.lib().smx_onehot_gates_fwd(dt(WihT), _p(tk32), _p(keep), pw, ldw, _p(bias), _p(Gx), rows, V, blank, G, _stream()),
            "smx_onehot_gates_fwd")
    _pe(tok)
    return Gx


def onehot_gates_wgrad(tk32, keep, dG, gW, V, blank):
    """gW (G, V - 1) fp32 [:, col(token[r])] += keep[r] dG[r, :], a fixed order per column (bit-reproducible)."""
    rows, G = dG.shape
    pg, ldg = _mat(dG)
    pw, ldw = _mat(gW)
    assert gW.dtype == torch.float32 and gW.shape == (G, V - 1)
    tok = _pb(f"onehot_gates_wgrad ({rows}x{G})", rows * G * (4 + _es(dG)))
    L.check(L.lib().smx_onehot_gates_wgrad(dt(dG), _p(tk32), _p(keep), pg, ldg, pw, ldw, rows, V, blank, G, _stream()),
            "smx_onehot_gates_wgrad")
    _pe(tok)


def lstm_fwd(Gx, Whh, h0, c0, B, U, save):
    """Gx (B U, 4H) fp32, W_hh (4H, H), h0 (B, H) in W_hh's dtype or None, c0 (B, H) fp32 or None -> (Y (B, U, H), hn (B, H), cn (B, H)
    fp32, saved); saved = (Hprev, gates, C) when `save`, else None."""
    H = Whh.shape[1]
    dev, T = Whh.device, Whh.dtype
    assert Gx.dtype == torch.float32 and Gx.is_contiguous() and Gx.shape == (B * U, 4 * H) and Whh.is_contiguous()
    assert (h0 is None or (h0.dtype == T and h0.is_contiguous())) and (c0 is None or (c0.dtype == torch.float32 and c0.is_contiguous()))
    Y = torch.empty((B, U, H), dtype=T, device=dev)
    hn = torch.empty((B, H), dtype=T, device=dev)
    cn = torch.empty((B, H), dtype=torch.float32, device=dev)
    saved = None
    if save:
        saved = (torch.empty((B, U, H), dtype=T, device=dev), torch.empty((B, U, 4 * H), dtype=torch.float32, device=dev),
                 torch.empty((B, U, H), dtype=torch.float32, device=dev))
    sv = saved or (None, None, None)
    tok = _pb(f"lstm_fwd {'bf16' if T == torch.bfloat16 else 'f32'} (B {B}, U {U}, H {H})", U * 4 * H * H * _es(Whh) + B * U * H * 36,
              2.0 * B * U * 4 * H * H)
    L.check(L.lib().smx_lstm_fwd(_DT[T], _p(Gx), _p(Whh), _p(h0), _p(c0), _p(Y), _p(sv[0]), _p(sv[1]), _p(sv[2]), _p(hn), _p(cn),
                                 B, U, H, _stream()), "smx_lstm_fwd")
    _pe(tok)
    return Y, hn, cn, saved


def lstm_bwd(dY, dhn, dcn, WhhT, gates, C, c0, B, U):
    """dY (B, U, H) in W_hh's dtype or None, dhn / dcn (B, H) fp32 or None, WhhT (H, 4H) -> (dG (B U, 4H), dh0, dc0 (B, H) fp32)."""
    H = WhhT.shape[0]
    dev, T = WhhT.device, WhhT.dtype
    assert WhhT.is_contiguous() and (dY is None or (dY.dtype == T and dY.is_contiguous()))
    assert all(t is None or (t.dtype == torch.float32 and t.is_contiguous()) for t in (dhn, dcn, c0))
    dG = torch.empty((B * U, 4 * H), dtype=T, device=dev)
    dh0 = torch.empty((B, H), dtype=torch.float32, device=dev)
    dc0 = torch.empty((B, H), dtype=torch.float32, device=dev)
    tok = _pb(f"lstm_bwd {'bf16' if T == torch.bfloat16 else 'f32'} (B {B}, U {U}, H {H})", U * 4 * H * H * _es(WhhT) + B * U * H * 40,
              2.0 * B * U * 4 * H * H)
    L.check(L.lib().smx_lstm_bwd(_DT[T], _p(dY), _p(dhn), _p(dcn), _p(WhhT), _p(gates), _p(C), _p(c0), _p(dG), _p(dc0), _p(dh0),
                                 B, U, H, _stream()), "smx_lstm_bwd")
    _pe(tok)
    return dG, dh0, dc0


# ---- the RNN language model's decode step and table gather (csrc/lstm_step.hip)
def lstm_step_ok(dtype, I, H):
    return dtype in _DT and bool(L.lib().smx_lstm_step_ok(_DT[dtype], I, H))


def lstm_step(x, Wih, Whh, bias, h, c, h_out=None, c_out=None, tokens=None):
    """One LSTM-cell step in one launch (smx_lstm_step).  tokens None: x (B, I) dense rows (unit stride along I); tokens (B) int32: x is
    the (V, I) table and row b of the input is x[tokens[b]] as stored (outside the table: zeros).  W_ih (4H, I), W_hh (4H, H) as
    torch.nn.LSTM stores them, bias (4H) fp32 = b_ih + b_hh, h (B, H) in the weights' dtype or None, c (B, H) fp32 or None.
    -> (h' (B, H), c' (B, H) fp32), written into h_out / c_out when given: buffers DISTINCT from h, c and x."""
    H, I = Whh.shape[1], Wih.shape[1]
    T, dev = Whh.dtype, Whh.device
    assert Whh.is_cuda, NO_CPU
    assert Wih.dtype == T and x.dtype == T and Wih.is_contiguous() and Whh.is_contiguous() and Wih.shape[0] == 4 * H and x.shape[1] == I
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == 4 * H
    B = x.shape[0] if tokens is None else tokens.numel()
    assert tokens is None or (tokens.dtype == torch.int32 and tokens.is_contiguous())
    assert (h is None or (h.dtype == T and h.is_contiguous() and h.shape == (B, H)))
    assert (c is None or (c.dtype == torch.float32 and c.is_contiguous() and c.shape == (B, H)))
    if h_out is None:
        h_out = torch.empty((B, H), dtype=T, device=dev)
    if c_out is None:
        c_out = torch.empty((B, H), dtype=torch.float32, device=dev)
    assert h_out.dtype == T and h_out.is_contiguous() and c_out.dtype == torch.float32 and c_out.is_contiguous()
    px, ldx = _mat(x)
    tok = _pb(f"lstm_step {'bf16' if T == torch.bfloat16 else 'f32'} (B {B}, I {I}, H {H})", 4 * H * (I + H) * _es(Whh) + B * (I + 2 * H) * _es(Whh) + 8 * B * H,
              2.0 * B * 4 * H * (I + H))
    L.check(L.lib().smx_lstm_step(_DT[T], px, ldx, _p(tokens), x.shape[0] if tokens is not None else 0, _p(Wih), _p(Whh), _p(bias),
                                  _p(h), _p(c), _p(h_out), _p(c_out), B, I, H, _stream()), "smx_lstm_step")
    _pe(tok)
    return h_out, c_out


def gather_rows(tokens, table):
    """tokens (...) integer, table (V, D) -> (..., D) = table[tokens] in the table's dtype (a token outside [0, V): a zero row)."""
    tk = _tokens_i32(tokens)
    V, D = table.shape
    Y = torch.empty((tk.numel(), D), dtype=table.dtype, device=table.device)
    pt, ldt = _mat(table)
    L.check(L.lib().smx_gather_rows(dt(table), _p(tk), pt, ldt, _p(Y), D, tk.numel(), V, D, _stream()), "smx_gather_rows")
    return Y.view(*tokens.shape, D)


# ---- greedy transducer decoding (csrc/greedy.hip).  Everything stays on the device: no call here synchronises with the host.
def greedy_ok(dtype, H, J, V):
    return dtype in _DT and bool(L.lib().smx_greedy_ok(_DT[dtype], H, J, V))


def greedy_start(bias, Wproj, B):
    """bias (4H) fp32 = b_ih + b_hh, W_proj (J, H) -> the state before the first frame: (h (B, H), c (B, H) fp32, pdec (B, J),
    frames_seen (B) int32 zeros)."""
    J, H = Wproj.shape
    dev, T = Wproj.device, Wproj.dtype
    assert bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == 4 * H and Wproj.is_contiguous()
    h = torch.empty((B, H), dtype=T, device=dev)
    c = torch.empty((B, H), dtype=torch.float32, device=dev)
    pdec = torch.empty((B, J), dtype=T, device=dev)
    seen = torch.empty((B,), dtype=torch.int32, device=dev)
    L.check(L.lib().smx_greedy_start(_DT[T], _p(bias), _p(Wproj), _p(h), _p(c), _p(pdec), _p(seen), B, H, J, _stream()), "smx_greedy_start")
    return h, c, pdec, seen


def greedy_decode(enc, in_len, WihT, bias, Whh, Wproj, Wlin, blin, state, logp, act, blank):
    """enc (B, T, J) with unit stride along J; in_len (B) int32 or None; state = (h, c, pdec, frames_seen), updated IN PLACE; logp (B)
    fp32, added into -> (tokens (B, T) int32 padded with -1, frames (B, T) int32, n_tok (B) int32)."""
    B, T, J = enc.shape
    h, c, pdec, seen = state
    H, V = Whh.shape[1], Wlin.shape[0]
    dev, DT = enc.device, enc.dtype
    assert enc.is_cuda, NO_CPU
    assert all(w.dtype == DT and w.is_contiguous() for w in (Whh, Wproj, Wlin, h, pdec)) and WihT.dtype == DT and WihT.stride(1) == 1
    assert all(t.dtype == torch.float32 and t.is_contiguous() for t in (bias, c, logp) + ((blin,) if blin is not None else ()))
    assert seen.dtype == torch.int32 and (in_len is None or (in_len.dtype == torch.int32 and in_len.is_contiguous()))
    assert h.shape == (B, H) and c.shape == (B, H) and pdec.shape == (B, J) and WihT.shape == (V - 1, 4 * H) and Wlin.shape[1] == J
    tokens = torch.empty((B, T), dtype=torch.int32, device=dev)
    frames = torch.empty((B, T), dtype=torch.int32, device=dev)
    n_tok = torch.empty((B,), dtype=torch.int32, device=dev)
    h_alt = torch.empty_like(h)
    ws = _workspace(L.lib().smx_greedy_workspace(B, V), dev, "greedy")
    tok = _pb(f"greedy_decode {'bf16' if DT == torch.bfloat16 else 'f32'} (B {B}, T {T}, V {V}, H {H}, J {J})",
              T * (V * J + 4 * H * H + J * H) * _es(enc), 2.0 * B * T * (V * J + 4 * H * H + J * H))
    L.check(L.lib().smx_greedy_decode(_DT[DT], _p(enc), enc.stride(0), enc.stride(1), _p(in_len), _p(WihT), WihT.stride(0), _p(bias),
                                      _p(Whh), _p(Wproj), _p(Wlin), _p(blin), _p(h), _p(h_alt), _p(c), _p(pdec), _p(seen), _p(tokens),
                                      _p(frames), _p(n_tok), _p(logp), B, T, H, J, V, act, blank, _p(ws), _stream()), "smx_greedy_decode")
    _pe(tok)
    return tokens, frames, n_tok


# ---- CTC greedy decoding (csrc/ctcdec.hip).  Everything stays on the device: no call here synchronises with the host.
def _row_outputs(N, device):
    return torch.empty((N,), dtype=torch.int32, device=device), torch.empty((N,), dtype=torch.float32, device=device)


def ctc_best_path(x2):
    """x2 (N, V) logits or log-probabilities with unit stride along V -> (tok (N) int32: lowest index of the row maximum, -1 for a
    row without a number; lp (N) fp32 = max - logsumexp): smx_ctc_best_path."""
    px, ldx = _mat(x2)
    N, V = x2.shape
    tok, lp = _row_outputs(N, x2.device)
    t = _pb(f"ctc_best_path {'bf16' if _es(x2) == 2 else 'f32'} ({N},{V})", N * V * _es(x2) + 8 * N)
    L.check(L.lib().smx_ctc_best_path(dt(x2), px, ldx, N, V, _p(tok), _p(lp), _stream()), "smx_ctc_best_path")
    _pe(t)
    return tok, lp


def ctc_head_ok(dtype, K, V):
    return dtype in _DT and bool(L.lib().smx_ctc_head_ok(_DT[dtype], K, V))


def ctc_head_best_path(x2, W, bias):
    """The same pair for z = x2 W^T + bias without storing z: x2 (N, K) and W (V, K) in one dtype, bias (V) fp32 or None
    (smx_ctc_head_best_path; the shapes of smx_ctc_head_ok)."""
    px, ldx = _mat(x2)
    N, K = x2.shape
    V = W.shape[0]
    assert W.is_cuda and W.dtype == x2.dtype and W.is_contiguous() and W.shape[1] == K
    assert bias is None or (bias.dtype == torch.float32 and bias.is_contiguous() and bias.numel() == V)
    tok, lp = _row_outputs(N, x2.device)
    ws = _workspace(L.lib().smx_ctc_head_workspace(N, V), x2.device, "ctc_head")
    t = _pb(f"ctc_head_best_path {'bf16' if _es(x2) == 2 else 'f32'} ({N},{K},{V})", (N * K + V * K) * _es(x2) + 8 * N, 2.0 * N * K * V)
    L.check(L.lib().smx_ctc_head_best_path(dt(x2), px, ldx, _p(W), _p(bias), N, K, V, _p(tok), _p(lp), _p(ws), _stream()),
            "smx_ctc_head_best_path")
    _pe(t)
    return tok, lp


def ctc_collapse(tok, lp, in_len, blank, start, state, tokens, frames):
    """tok int32 / lp fp32 (B, T) with one row stride; in_len (B) int32 or None; start (B) uint8 or None; state = (prev, seen, n_tok,
    score), updated IN PLACE; tokens / frames (B, cap) int32, appended to at n_tok (smx_ctc_collapse)."""
    B, T = tok.shape
    prev, seen, n_tok, score = state
    assert tok.is_cuda, NO_CPU
    assert tok.dtype == torch.int32 and lp.dtype == torch.float32 and lp.shape == tok.shape
    assert T == 0 or (tok.stride(1) == 1 and lp.stride(1) == 1 and (B == 1 or tok.stride(0) == lp.stride(0)))
    assert all(t.dtype == torch.int32 and t.is_contiguous() and t.shape == (B,) for t in (prev, seen, n_tok))
    assert score.dtype == torch.float32 and score.is_contiguous() and score.shape == (B,)
    assert in_len is None or (in_len.dtype == torch.int32 and in_len.is_contiguous() and in_len.shape == (B,))
    assert start is None or (start.dtype == torch.uint8 and start.is_contiguous() and start.shape == (B,))
    assert tokens.dtype == torch.int32 and frames.dtype == torch.int32 and tokens.is_contiguous() and frames.is_contiguous()
    assert tokens.dim() == 2 and tokens.shape[0] == B and frames.shape == tokens.shape
    a = L.CtcCollapse(tok=_p(tok), lp=_p(lp), ld=max(tok.stride(0), T) if B > 1 else T, in_len=_p(in_len), start=_p(start), prev=_p(prev),
                      seen=_p(seen), n_tok=_p(n_tok), score=_p(score), tokens=_p(tokens), frames=_p(frames), B=B, T=T, blank=int(blank),
                      cap=tokens.shape[1])
    t = _pb(f"ctc_collapse (B {B}, T {T})", 8 * B * T)
    L.check(L.lib().smx_ctc_collapse(ctypes.byref(a), _stream()), "smx_ctc_collapse")
    _pe(t)


_CSGU_DROP_FUSE = True   # (round 4: A/B knob SMX_CSGU_DROP_FUSE removed)     # (read once, like the library's own knobs)
_STEP_COUNTER = None          # the training loop's device step counter (held HERE, in the Python host; libsmx has no such state)


def _epoch():
    return None if _STEP_COUNTER is None else ctypes.c_void_p(_STEP_COUNTER.data_ptr())


def set_step_counter(counter):
    """Use (or stop using, with None) a device step counter - an int64 tensor of one element - in every dropout seed and
    AdamW bias correction issued through this module.  The library takes the counter as an explicit argument of each
    call (include/smx.h: `epoch`, smx_epilogue.epoch, `step_dev`); this module-level variable is the host's training
    loop state, the place torch keeps its own default generator."""
    global _STEP_COUNTER
    if counter is not None:
        assert counter.is_cuda and counter.dtype == torch.int64 and counter.numel() == 1
    _STEP_COUNTER = counter


def step_counter_add(counter, inc=1):
    L.check(L.lib().smx_step_counter_add(_p(counter), inc, _stream()), "smx_step_counter_add")


def capture_id():
    """Id of the hipGraph capture the current stream records into; 0 when it is not capturing (smx_stream_capture_id)."""
    if not torch.cuda.is_current_stream_capturing():
        return 0
    cid = ctypes.c_uint64(0)
    L.check(L.lib().smx_stream_capture_id(_stream(), ctypes.byref(cid)), "smx_stream_capture_id")
    return int(cid.value) or -1


def sumsq(x, out):
    ws = _workspace(L.lib().smx_sumsq_workspace(), x.device, slot=6)
    L.check(L.lib().smx_sumsq(_p(x), x.numel(), _p(out), _p(ws), _stream()), "smx_sumsq")


def clip_factor(sumsq_t, max_norm, inv_scale, out):
    L.check(L.lib().smx_clip_factor(_p(sumsq_t), max_norm, inv_scale, _p(out), _stream()), "smx_clip_factor")


# ---- front-end -----------------------------------------------------------------------------------------
def frame_window(wav, window, T, n_fft, hop):
    B, Lw = wav.shape
    out = torch.empty((B * T, n_fft), dtype=torch.float32, device=wav.device)
    L.check(L.lib().smx_frame_window(_p(wav), wav.stride(0), _p(window), _p(out), B, Lw, T, n_fft, hop, _stream()),
            "smx_frame_window")
    return out


def mel_db(spec, im_off, fb, B, T, amin, top_db, out_dtype):
    n_mels, n_bins = fb.shape
    out = torch.empty((B, T, n_mels), dtype=out_dtype, device=spec.device)
    ws = _workspace(L.lib().smx_fbank_workspace(B, T, n_mels), spec.device, slot=5)
    L.check(L.lib().smx_mel_db(_DT[out_dtype], _p(spec), spec.stride(0), im_off, _p(fb), n_bins, n_mels, amin, top_db, _p(out),
                               B, T, _p(ws), _stream()), "smx_mel_db")
    return out


def im2col_s2(x, Kp):
    B, T, F_, C = x.shape
    T2, F2 = (T + 1) // 2, (F_ + 1) // 2
    col = torch.empty((B * T2 * F2, Kp), dtype=x.dtype, device=x.device)
    L.check(L.lib().smx_im2col_s2(dt(x), _p(x), _p(col), B, T, F_, C, Kp, _stream()), "smx_im2col_s2")
    return col


def dft_frames(wav_padded, basis_cos, basis_sin, spec, im_off, B, T, n_fft, hop):
    """spec (B*T, lds) <- DFT of the overlapping frames of the zero-padded waveform rows (smx_dft_frames: no frame matrix, folded
    cosine / sine halves)."""
    tok = _pb(f"dft_frames ({B},{T}) n_fft={n_fft}", wav_padded.numel() * 4 + spec.numel() * 4, 2.0 * B * T * n_fft * (n_fft / 2 + 1))
    L.check(L.lib().smx_dft_frames(_p(wav_padded), wav_padded.stride(0), _p(basis_cos), _p(basis_sin), _p(spec), spec.stride(0), im_off,
                                   B, T, n_fft, hop, basis_cos.shape[0], _stream()), "smx_dft_frames")
    _pe(tok)


def conv1_ln_ok(x, O):
    """Does the fused first conv block (smx_conv1_ln_fwd / _bwd) take this input?  x (B, T, F) contiguous, one input channel."""
    B, T, F_ = x.shape
    return (x.dtype in (torch.bfloat16, torch.float32) and x.is_contiguous() and O == 64 and F_ % 16 == 0 and 16 <= F_ <= 160
            and T >= 2 and L.lib().smx_conv1_ln_workspace(B, T, F_, O) > 0)


def conv1_ln_fwd(x, w9, bias, gamma, beta, eps, act, need_stats=True):
    """a = act(LayerNorm(conv3x3_s2_reflect(x) + bias) * gamma + beta) in one pass: x (B,T,F) -> (B*T2, (F/2)*O), stats."""
    B, T, F_ = x.shape
    O = w9.shape[0]
    T2 = (T + 1) // 2
    y = torch.empty((B * T2, (F_ // 2) * O), dtype=x.dtype, device=x.device)
    stats = torch.empty((B * T2, 2), dtype=torch.float32, device=x.device) if need_stats else None
    tok = _pb(f"conv1_ln_fwd ({B},{T},{F_})->{O}", x.numel() * _es(x) + y.numel() * _es(y))
    L.check(L.lib().smx_conv1_ln_fwd(dt(x), _p(x), _p(w9), _p(bias), _p(gamma), _p(beta), eps, act, _p(y), _p(stats), B, T, F_, O,
                                     _stream()), "smx_conv1_ln_fwd")
    _pe(tok)
    return y, stats


def conv1_ln_bwd(da, x, w9, bias, gamma, beta, stats, act):
    """Gradients of the fused first conv block from dA and x: a flat fp32 tensor [dgamma | dbeta | dW9 (O,9) | dbias]."""
    B, T, F_ = x.shape
    O = w9.shape[0]
    D = (F_ // 2) * O
    grads = torch.zeros(2 * D + O * 10, dtype=torch.float32, device=x.device)
    ws = _workspace(L.lib().smx_conv1_ln_workspace(B, T, F_, O), x.device, slot=7)
    tok = _pb(f"conv1_ln_bwd ({B},{T},{F_})->{O}", da.numel() * _es(da) + x.numel() * _es(x))
    L.check(L.lib().smx_conv1_ln_bwd(dt(x), _p(da), _p(x), _p(w9), _p(bias), _p(gamma), _p(beta), _p(stats), act, _p(grads), _p(ws),
                                     B, T, F_, O, _stream()), "smx_conv1_ln_bwd")
    _pe(tok)
    return grads


def linear_k16(x, W, bias):
    """y = x W^T + bias for K = 16 on the VALU (smx_linear_k16_fwd), or None when the shape is not the kernel's."""
    N, K = x.shape
    M = W.shape[0]
    if not (x.dtype == torch.bfloat16 and W.dtype == torch.bfloat16 and K == 16 and x.is_contiguous() and W.is_contiguous()
            and M % 8 == 0 and 256 % (M // 8) == 0):
        return None
    y = torch.empty((N, M), dtype=x.dtype, device=x.device)
    tok = _pb(f"linear_k16 ({N}x16)x(16x{M})", N * (K + M) * 2)
    L.check(L.lib().smx_linear_k16_fwd(dt(x), _p(x), _p(W), _p(bias), _p(y), N, M, _stream()), "smx_linear_k16_fwd")
    _pe(tok)
    return y


def conv2d_s2_direct_ok(x, O):
    """Do the patch-matrix-free kernels (smx_conv2d_s2_fwd / _wgrad) take this block input x (B, T, F, C)?"""
    B, T, F_, C = x.shape
    return (x.dtype == torch.bfloat16 and x.is_contiguous() and C == 64 and O % 8 == 0 and T >= 2 and F_ >= 2
            and x.numel() * 2 < (1 << 31) and x.data_ptr() % 16 == 0)


def conv2d_s2_fwd(x, wg, bias, O):
    """y (B*T2*F2, O) = conv3x3_s2_reflect(x) + bias with the GEMM gathering its operand from x (B,T,F,64) in place."""
    B, T, F_, C = x.shape
    rows = B * ((T + 1) // 2) * ((F_ + 1) // 2)
    y = torch.empty((rows, O), dtype=x.dtype, device=x.device)
    tok = _pb(f"conv2d_s2_fwd ({B},{T},{F_},{C})->{O}", x.numel() * 2 + y.numel() * 2, 2.0 * rows * O * 9 * C)
    L.check(L.lib().smx_conv2d_s2_fwd(dt(x), _p(x), _p(wg), _p(bias), _p(y), B, T, F_, C, O, wg.shape[1], _stream()), "smx_conv2d_s2_fwd")
    _pe(tok)
    return y


def conv2d_s2_wgrad(dy, x, gw, gbias):
    """gw (O, Kp) fp32 += dy^T patches(x), gbias (O) += column sums of dy (slab split-K, fixed-order reduction)."""
    B, T, F_, C = x.shape
    O = dy.shape[1]
    ws = _workspace(L.lib().smx_conv2d_s2_wgrad_workspace(B, T, F_, C, O), x.device, slot=6)
    tok = _pb(f"conv2d_s2_wgrad ({B},{T},{F_},{C})->{O}", x.numel() * 2 + dy.numel() * 2, 2.0 * dy.shape[0] * O * 9 * C)
    L.check(L.lib().smx_conv2d_s2_wgrad(dt(x), _p(dy), _p(x), _p(gw), _p(gbias), B, T, F_, C, O, gw.shape[1], _p(ws), _stream()),
            "smx_conv2d_s2_wgrad")
    _pe(tok)


def conv2d_s2_dgrad_ok(dy, C, O, T, F_):
    """Does the direct dgrad kernel (smx_conv2d_s2_dgrad) take this block?  (bf16, 64 -> 32 channels: the recipe's second)"""
    return dy.dtype == torch.bfloat16 and C == 64 and O == 32 and T >= 4 and F_ >= 4 and dy.numel() * 2 < (1 << 31)


def conv2d_s2_dgrad(dy, wg, B, T, F_, C):
    """dx (B,T,F,C) of the 3x3 / stride 2 / reflect-pad-1 convolution from dy (B*T2*F2, O) and the GEMM-layout weight."""
    dx = torch.empty((B, T, F_, C), dtype=dy.dtype, device=dy.device)
    tok = _pb(f"conv2d_s2_dgrad ({B},{T},{F_},{C})", dx.numel() * 2 + dy.numel() * 2)
    L.check(L.lib().smx_conv2d_s2_dgrad(dt(dy), _p(dy), _p(wg), _p(dx), B, T, F_, C, dy.shape[1], wg.shape[1], _stream()),
            "smx_conv2d_s2_dgrad")
    _pe(tok)
    return dx


def col2im_s2(dcol, B, T, F_, C):
    dx = torch.empty((B, T, F_, C), dtype=dcol.dtype, device=dcol.device)
    L.check(L.lib().smx_col2im_s2(dt(dcol), _p(dcol), _p(dx), B, T, F_, C, dcol.shape[1], _stream()), "smx_col2im_s2")
    return dx


# ---- scaled-dot-product attention (csrc/attention.hip).  q (B, L, H, D), k / v (B, S, H, D): 4-D views with unit stride along D and
# any batch / row / head strides (views of a packed (B, L, 3, H, D) or (B, S, 2, H, D) projection output are not copied).
def _attn_operand(t, B, R, H, D, what):
    if t is None:
        return L.AttnOperand()
    if not t.is_cuda:
        raise RuntimeError(NO_CPU)
    assert t.dim() == 4 and tuple(t.shape) == (B, R, H, D), f"attention: {what} must be ({B}, {R}, {H}, {D}), got {tuple(t.shape)}"
    sb, sr, sh, sd = t.stride()
    # (the stride of a size-1 dimension is arbitrary in torch and never multiplied by anything but 0: hand the kernels 0)
    return L.AttnOperand(t.data_ptr(), sb if B > 1 else 0, sr if R > 1 else 0, sh if H > 1 else 0, sd)


def _attn_args(q, k, v, attn_bias, key_pad, causal, scale, drop_p, seed):
    B, Lq, H, D = q.shape
    S = k.shape[1]
    a = L.AttnArgs(dtype=dt(q), causal=int(bool(causal)), B=B, L=Lq, S=S, H=H, D=D, scale=float(scale), drop_p=float(drop_p),
                   drop_seed=int(seed or 0) & 0xFFFFFFFFFFFFFFFF)
    assert k.dtype == q.dtype and (v is None or v.dtype == q.dtype), "attention: q, k, v must share a dtype"
    a.q, a.k, a.v = _attn_operand(q, B, Lq, H, D, "q"), _attn_operand(k, B, S, H, D, "k"), _attn_operand(v, B, S, H, D, "v")
    if attn_bias is not None:
        assert attn_bias.is_cuda and attn_bias.dtype == torch.float32 and tuple(attn_bias.shape) == (Lq, S) and (S == 1 or attn_bias.stride(1) == 1)
        a.attn_bias, a.ldbias = attn_bias.data_ptr(), attn_bias.stride(0) if Lq > 1 else max(attn_bias.stride(0), S)
    if key_pad is not None:
        assert key_pad.is_cuda and key_pad.dtype == torch.uint8 and tuple(key_pad.shape) == (B, S) and (S == 1 or key_pad.stride(1) == 1)
        a.key_pad, a.ldpad = key_pad.data_ptr(), key_pad.stride(0) if B > 1 else max(key_pad.stride(0), S)
    a.epoch = _epoch() if drop_p > 0.0 else None
    return a, (B, Lq, S, H, D)


def _attn_name(what, q, dims, causal, drop_p):
    return f"{what} {'bf16' if _es(q) == 2 else 'f32'} (B {dims[0]}, L {dims[1]}, S {dims[2]}, H {dims[3]}, D {dims[4]})" + (
        " causal" if causal else "") + (f" p={drop_p}" if drop_p > 0.0 else "")


def attention_fwd(q, k, v, attn_bias=None, key_pad=None, causal=False, scale=None, drop_p=0.0, seed=0, out=None):
    """-> (o (B, L, H, D) in q's dtype, lse (B, H, L) fp32): smx_attn_fwd, one launch.  attn_bias fp32 (L, S) additive (-inf = masked),
    key_pad uint8 (B, S) (non-zero = masked), seed: the dropout site's seed (the device step counter is mixed in when one is set)."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    a, (B, Lq, S, H, D) = _attn_args(q, k, v, attn_bias, key_pad, causal, scale, drop_p, seed)
    if out is None:
        out = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device)
    lse = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    a.o, a.lse = _attn_operand(out, B, Lq, H, D, "out"), lse.data_ptr()
    tok = _pb(_attn_name("attn_fwd", q, (B, Lq, S, H, D), causal, drop_p), (2 * B * Lq + 2 * B * S) * H * D * _es(q), 4.0 * B * H * Lq * S * D)
    L.check(L.lib().smx_attn_fwd(ctypes.byref(a), _stream()), "smx_attn_fwd")
    _pe(tok)
    return out, lse


def attention_bwd(do, q, k, v, o, lse, attn_bias=None, key_pad=None, causal=False, scale=None, drop_p=0.0, seed=0,
                  dq=None, dk=None, dv=None):
    """-> (dq, dk, dv): smx_attn_bwd (two launches, no atomics; `o` is accepted for symmetry with the saved tensors and not read).  dq / dk / dv may be views into a packed gradient buffer; every
    element of them is written."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    a, (B, Lq, S, H, D) = _attn_args(q, k, v, attn_bias, key_pad, causal, scale, drop_p, seed)
    dq = torch.empty((B, Lq, H, D), dtype=q.dtype, device=q.device) if dq is None else dq
    dk = torch.empty((B, S, H, D), dtype=q.dtype, device=q.device) if dk is None else dk
    dv = torch.empty((B, S, H, D), dtype=q.dtype, device=q.device) if dv is None else dv
    assert do.dtype == q.dtype and o.dtype == q.dtype and dq.dtype == q.dtype and dk.dtype == q.dtype and dv.dtype == q.dtype
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Lq) and lse.is_contiguous()
    delta = torch.empty((B, H, Lq), dtype=torch.float32, device=q.device)
    a.o, a.dO = _attn_operand(o, B, Lq, H, D, "o"), _attn_operand(do, B, Lq, H, D, "do")
    a.dq, a.dk, a.dv = _attn_operand(dq, B, Lq, H, D, "dq"), _attn_operand(dk, B, S, H, D, "dk"), _attn_operand(dv, B, S, H, D, "dv")
    a.lse, a.delta = lse.data_ptr(), delta.data_ptr()
    tok = _pb(_attn_name("attn_bwd", q, (B, Lq, S, H, D), causal, drop_p), (4 * B * Lq + 4 * B * S) * H * D * _es(q), 16.0 * B * H * Lq * S * D)
    L.check(L.lib().smx_attn_bwd(ctypes.byref(a), _stream()), "smx_attn_bwd")
    _pe(tok)
    return dq, dk, dv


def attention_weights(q, k, lse, attn_bias=None, key_pad=None, causal=False, scale=None, drop_p=0.0, seed=0):
    """-> W (B, L, S) fp32, the head-averaged (dropped, when drop_p > 0) probabilities: smx_attn_weights, a launch of its own."""
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    a, (B, Lq, S, H, D) = _attn_args(q, k, None, attn_bias, key_pad, causal, scale, drop_p, seed)
    assert lse.dtype == torch.float32 and tuple(lse.shape) == (B, H, Lq) and lse.is_contiguous()
    W = torch.empty((B, Lq, S), dtype=torch.float32, device=q.device)
    a.lse, a.weights, a.w_sb, a.ldw = lse.data_ptr(), W.data_ptr(), Lq * S, S
    tok = _pb(_attn_name("attn_weights", q, (B, Lq, S, H, D), causal, drop_p), (B * Lq + B * S) * H * D * _es(q) + 4 * B * Lq * S,
              2.0 * B * H * Lq * S * D)
    L.check(L.lib().smx_attn_weights(ctypes.byref(a), _stream()), "smx_attn_weights")
    _pe(tok)
    return W


def attention_plan(B, Lq, S, H, D, dtype=torch.float32, which=L.ATTN_FWD):
    """smx_attn_plan_query for a problem size (needs no GPU): a dict of the pass's tile rows, key-tile width, D chunk, LDS bytes,
    threads, launches and grid.  Raises where the library refuses the problem (head dimension, dtype)."""
    a = L.AttnArgs(dtype=_DT.get(dtype, -1), B=B, L=Lq, S=S, H=H, D=D, scale=D ** -0.5)
    plan = L.AttnPlan()
    L.check(L.lib().smx_attn_plan_query(ctypes.byref(a), int(which), ctypes.byref(plan)), "smx_attn_plan_query")
    return dict(rows=plan.rows, key_tile=plan.key_tile, d_chunk=plan.d_chunk, lds_bytes=plan.lds_bytes, threads=plan.threads,
                launches=plan.launches, grid=tuple(plan.grid))


# ---- target embedding of the seq2seq decoder (csrc/tgt_embed.hip).  One launch per direction; neither synchronises with the host.
def tgt_embed_fwd(tokens, table, pe, pad_idx=0, out_dtype=torch.float32, out=None, key_pad=None):
    """tokens (B, U) integer, table (V, d) fp32, pe (>= U, d) fp32 (rows [0, U) are read) -> (y (B, U, d) in out_dtype =
    table[tokens] * sqrt(d) + pe[u], key_pad (B, U) bool = tokens == pad_idx).  A token outside [0, V): y = pe[u], flag False.
    out / key_pad: destinations to write instead of fresh ones ((B U, d) rows view in out_dtype, (B U) uint8)."""
    if not (tokens.is_cuda and table.is_cuda and pe.is_cuda):
        raise RuntimeError(NO_CPU)
    assert tokens.dim() == 2 and table.dim() == 2 and table.dtype == torch.float32 and pe.dtype == torch.float32
    B, U = tokens.shape
    V, D = table.shape
    assert pe.dim() == 2 and pe.shape[0] >= U and pe.shape[1] == D, f"tgt_embed: pe must hold {U} rows of {D}, got {tuple(pe.shape)}"
    tk = _tokens_i32(tokens)
    y = torch.empty((B * U, D), dtype=out_dtype, device=table.device) if out is None else out
    flags = torch.empty((B * U,), dtype=torch.uint8, device=table.device) if key_pad is None else key_pad
    assert y.dtype == out_dtype and tuple(y.shape) == (B * U, D) and flags.dtype == torch.uint8 and flags.numel() == B * U and flags.is_contiguous()
    pt, ldt = _mat(table)
    pp, ldp = _mat(pe)
    py, ldy = _mat(y)
    tok = _pb(f"tgt_embed_fwd {'bf16' if out_dtype == torch.bfloat16 else 'f32'} ({B * U}x{D}, V {V})", B * U * (D * (8 + _es(y)) + 5))
    L.check(L.lib().smx_tgt_embed_fwd(_DT[out_dtype], _p(tk), pt, ldt, pp, ldp, py, ldy, _p(flags), B * U, U, V, D, int(pad_idx), _stream()),
            "smx_tgt_embed_fwd")
    _pe(tok)
    return y.view(B, U, D), flags.view(B, U).view(torch.bool)


def tgt_embed_bwd(tokens, dy, gtable, pad_idx=0):
    """gtable (V, d) fp32 += sqrt(d) * sum over the rows r with tokens[r] == v of dy[r] (dy (B U, d) or (B, U, d), float32 or
    bfloat16), rows added in ascending r, no atomics.  Row pad_idx and tokens outside [0, V) receive nothing."""
    if not (tokens.is_cuda and dy.is_cuda and gtable.is_cuda):
        raise RuntimeError(NO_CPU)
    V, D = gtable.shape
    assert gtable.dtype == torch.float32
    dy2 = rows2d(dy)
    tk = _tokens_i32(tokens)
    assert dy2.shape == (tk.numel(), D), f"tgt_embed_bwd: dy must be ({tk.numel()}, {D}), got {tuple(dy2.shape)}"
    pd, ldd = _mat(dy2)
    pg, ldg = _mat(gtable)
    tok = _pb(f"tgt_embed_bwd {'bf16' if _es(dy2) == 2 else 'f32'} ({tk.numel()}x{D}, V {V})", tk.numel() * (D * (_es(dy2) + 8) + 4))
    L.check(L.lib().smx_tgt_embed_bwd(dt(dy2), _p(tk), pd, ldd, pg, ldg, tk.numel(), V, D, int(pad_idx), _stream()), "smx_tgt_embed_bwd")
    _pe(tok)
    return gtable


# ---- one KV-cached decoding step (csrc/attn_step.hip).  Positions are device counters; no call here synchronises with the host.
def _step_operand(t, B, H, D, what, cap=None):
    """(B, H, D), or a cache (B, cap, H, D), as an smx_attn_operand."""
    if t is None:
        return L.AttnOperand()
    if not t.is_cuda:
        raise RuntimeError(NO_CPU)
    want = (B, H, D) if cap is None else (B, cap, H, D)
    assert tuple(t.shape) == want, f"attention_step: {what} must be {want}, got {tuple(t.shape)}"
    st = t.stride()
    sb, sh, sd = st[0], st[-2], st[-1]
    return L.AttnOperand(t.data_ptr(), sb if B > 1 else 0, (st[1] if cap > 1 else 0) if cap is not None else 0, sh if H > 1 else 0, sd)


def attention_step_plan(B, H, D, cap, dtype=torch.float32, kv_div=None):
    """smx_attn_step_plan_query for a problem size (needs no GPU): a dict of the launch geometry.  Raises where the library refuses.
    kv_div: ask smx_attn_step_rows_plan_query, the indexed entry's (B = the query rows), instead."""
    a = L.AttnStepArgs(dtype=_DT.get(dtype, -1), B=B, H=H, D=D, cap=cap, scale=1.0)
    p = L.AttnStepPlan()
    if kv_div is None:
        L.check(L.lib().smx_attn_step_plan_query(ctypes.byref(a), ctypes.byref(p)), "smx_attn_step_plan_query")
    else:
        r = L.AttnStepRowsArgs(s=a, kv_div=int(kv_div))
        L.check(L.lib().smx_attn_step_rows_plan_query(ctypes.byref(r), ctypes.byref(p)), "smx_attn_step_rows_plan_query")
    return dict(lanes_per_key=p.lanes_per_key, keys_per_wave=p.keys_per_wave, waves=p.waves, threads=p.threads, splits=p.splits,
                chunk=p.chunk, launches=p.launches, lds_bytes=p.lds_bytes, grid=tuple(p.grid), workspace_bytes=p.workspace_bytes)


_STEP_WS = {}   # (B, H, D, cap, dtype code) -> workspace floats of smx_attn_step (a function of the sizes alone: asked once)


def attention_step_workspace(B, H, D, cap, dtype=torch.float32):
    """fp32 elements of workspace ops.attention_step needs at these sizes (0: a single launch); the plan query runs once per size."""
    key = (B, H, D, cap, _DT.get(dtype, -1))
    n = _STEP_WS.get(key)
    if n is None:
        n = _STEP_WS[key] = attention_step_plan(B, H, D, cap, dtype)["workspace_bytes"] // 4
    return n


def attention_step(q, K, V, n_keys=None, k_new=None, v_new=None, scale=None, out=None, workspace=None, anc=None, kv_div=None):
    """One query row per (batch row, head) over a cache: q (B, H, D), K / V (B, cap, H, D), n_keys (B) int32 on the device (None:
    all cap keys) -> o (B, H, D) in q's dtype (smx_attn_step).  With k_new / v_new (B, H, D) the call first stores them into cache slot
    n_keys[b] - 1.  All operands are read in place through their strides (unit stride along D, 16-byte aligned rows).  out / workspace
    (fp32, at least attention_step_workspace elements): buffers the caller owns - a decoding state hands in its own, so a step
    allocates nothing here; fresh ones otherwise.
    anc / kv_div (beam search; smx_attn_step_rows, the same arithmetic over an indexed cache): with kv_div = W query row r reads cache
    row and n_keys entry r // W, so K / V hold B / W rows and n_keys as many entries; with anc (B, cap) int32 on the device key
    j < n - 1 of row r is read from cache row anc[r, j] (an entry outside [0, B) removes the key).  With neither, smx_attn_step."""
    if not (q.is_cuda and K.is_cuda and V.is_cuda):
        raise RuntimeError(NO_CPU)
    B, H, D = q.shape
    cap = K.shape[1]
    rows = anc is not None or kv_div is not None
    kv_div = 1 if kv_div is None else int(kv_div)
    Bc = -(-B // kv_div) if kv_div >= 1 else B                # cache rows (the library refuses kv_div < 1)
    assert K.dtype == q.dtype and V.dtype == q.dtype and (k_new is None) == (v_new is None)
    assert k_new is None or (k_new.dtype == q.dtype and v_new.dtype == q.dtype)
    assert n_keys is None or (n_keys.is_cuda and n_keys.dtype == torch.int32 and n_keys.is_contiguous() and n_keys.shape == (Bc,))
    assert anc is None or (anc.is_cuda and anc.dtype == torch.int32 and tuple(anc.shape) == (B, cap) and anc.stride(1) == 1)
    if out is None:
        out = torch.empty((B, H, D), dtype=q.dtype, device=q.device)
    a = L.AttnStepArgs(dtype=dt(q), B=B, H=H, D=D, cap=cap, scale=float(D ** -0.5 if scale is None else scale), n_keys=_p(n_keys))
    a.q, a.o = _step_operand(q, B, H, D, "q"), _step_operand(out, B, H, D, "out")
    a.k_new, a.v_new = _step_operand(k_new, B, H, D, "k_new"), _step_operand(v_new, B, H, D, "v_new")
    a.K, a.V = _step_operand(K, Bc, H, D, "K", cap), _step_operand(V, Bc, H, D, "V", cap)
    need = attention_step_workspace(B, H, D, cap, q.dtype)
    if need:
        if workspace is None:
            workspace = torch.empty((need,), dtype=torch.float32, device=q.device)
        assert workspace.is_cuda and workspace.dtype == torch.float32 and workspace.is_contiguous() and workspace.numel() >= need
        a.workspace = workspace.data_ptr()
    tok = _pb(f"attn_step {'bf16' if _es(q) == 2 else 'f32'} (B {B}, cap {cap}, H {H}, D {D})" + (" self" if k_new is not None else "") +
              (" rows" if rows else ""), 2 * B * cap * H * D * _es(q), 4.0 * B * H * cap * D)
    if rows:
        r = L.AttnStepRowsArgs(s=a, anc=_p(anc), ld_anc=anc.stride(0) if anc is not None else 0, kv_div=kv_div)
        L.check(L.lib().smx_attn_step_rows(ctypes.byref(r), _stream()), "smx_attn_step_rows")
    else:
        L.check(L.lib().smx_attn_step(ctypes.byref(a), _stream()), "smx_attn_step")
    _pe(tok)
    return out


def s2s_embed_step(tok, table, pe, pos, done, max_pos, out_dtype=torch.float32, out=None):
    """y (B, d) = table[tok] * sqrt(d) + pe[pos] in out_dtype, then pos += 1 on the rows with done == 0 (smx_s2s_embed_step): tok (B)
    int32, table (V, d) fp32, pe (>= max_pos, d) fp32 or None, pos (B) int32 and done (B) uint8 on the device, updated IN PLACE.  A row
    at pos >= max_pos is marked done instead of advanced."""
    if not (tok.is_cuda and table.is_cuda and pos.is_cuda and done.is_cuda and (pe is None or pe.is_cuda)):
        raise RuntimeError(NO_CPU)
    B = tok.shape[0]
    V, D = table.shape
    assert tok.dtype == torch.int32 and tok.is_contiguous() and tok.dim() == 1
    assert pos.dtype == torch.int32 and pos.is_contiguous() and pos.shape == (B,) and done.dtype == torch.uint8 and done.is_contiguous() and done.shape == (B,)
    assert table.dtype == torch.float32 and (pe is None or (pe.dtype == torch.float32 and pe.dim() == 2 and pe.shape[1] == D and pe.shape[0] >= max_pos))
    y = torch.empty((B, D), dtype=out_dtype, device=table.device) if out is None else out
    assert y.dtype == out_dtype and tuple(y.shape) == (B, D)
    pt, ldt = _mat(table)
    pp, ldp = _mat(pe) if pe is not None else (None, 0)
    py, ldy = _mat(y)
    L.check(L.lib().smx_s2s_embed_step(_DT[out_dtype], _p(tok), pt, ldt, pp, ldp, py, ldy, _p(pos), _p(done), B, V, D, int(max_pos), _stream()),
            "smx_s2s_embed_step")
    return y


def s2s_select(logits, tok, done, n_tok, score, tokens, logp_tok, eos, min_steps=0, inv_temp=1.0, forced=None):
    """The token selection of one search step over logits (B, V) (smx_s2s_select): arg-max (or forced (B) int32), its log-probability at
    temperature 1 / inv_temp, appended to tokens / logp_tok (B, cap) at n_tok; score, n_tok, done, tok updated IN PLACE on the rows with
    done == 0."""
    if not logits.is_cuda:
        raise RuntimeError(NO_CPU)
    pz, ldz = _mat(logits)
    B, V = logits.shape
    cap = tokens.shape[1]
    assert all(t.is_cuda and t.is_contiguous() for t in (tok, done, n_tok, score, tokens, logp_tok))
    assert tok.dtype == torch.int32 and n_tok.dtype == torch.int32 and tokens.dtype == torch.int32 and done.dtype == torch.uint8
    assert score.dtype == torch.float32 and logp_tok.dtype == torch.float32
    assert tok.shape == (B,) and done.shape == (B,) and n_tok.shape == (B,) and score.shape == (B,) and tuple(tokens.shape) == (B, cap) and tuple(logp_tok.shape) == (B, cap)
    assert forced is None or (forced.is_cuda and forced.dtype == torch.int32 and forced.is_contiguous() and forced.shape == (B,))
    a = L.S2SSelectArgs(logits=pz, ldz=ldz, forced=_p(forced), tok=_p(tok), done=_p(done), n_tok=_p(n_tok), score=_p(score), tokens=_p(tokens),
                        logp_tok=_p(logp_tok), inv_temp=float(inv_temp), dtype=dt(logits), B=B, V=V, cap=cap, eos=int(eos), min_steps=int(min_steps))
    L.check(L.lib().smx_s2s_select(ctypes.byref(a), _stream()), "smx_s2s_select")


def s2s_beam_select(logits, st, eos, min_steps=0, inv_temp=1.0, length_norm=True, extra=None):
    """The selection of one beam-search step over logits (B W, V) (smx_s2s_beam_select): per utterance the W best of its rows'
    candidates score + log-probability (+ extra (B W, V) fp32, the scorer hook) become its new slots, the ones that end go to its
    pool.  st: the beam part of a Transformer.DecodeState (tok, score, row_done, done, n_tok, tokens, logp_tok, anc, the scratch
    tables, the candidate workspace, the pool and the result), all updated IN PLACE; two launches, the same at every step."""
    if not logits.is_cuda:
        raise RuntimeError(NO_CPU)
    pz, ldz = _mat(logits)
    R, V = logits.shape
    B, W, cap = st.B, st.beam, st.cap
    assert R == B * W, f"s2s_beam_select: logits must have B W = {B * W} rows, got {R}"
    px, ldx = (None, 0)
    if extra is not None:
        assert extra.is_cuda and extra.dtype == torch.float32 and tuple(extra.shape) == (R, V)
        px, ldx = _mat(extra)
    shapes = {"tok": ((R,), torch.int32), "score": ((R,), torch.float32), "row_done": ((R,), torch.uint8), "done": ((B,), torch.uint8),
              "n_tok": ((B,), torch.int32), "tokens": ((R, cap), torch.int32), "logp_tok": ((R, cap), torch.float32),
              "anc": ((R, cap), torch.int32), "s_tokens": ((R, cap), torch.int32), "s_logp": ((R, cap), torch.float32),
              "s_anc": ((R, cap), torch.int32), "cand_val": ((R, W), torch.float32), "cand_lp": ((R, W), torch.float32),
              "cand_idx": ((R, W), torch.int32), "cand_n": ((R,), torch.int32), "pool_tokens": ((B, W, cap), torch.int32),
              "pool_logp": ((B, W, cap), torch.float32), "pool_len": ((B, W), torch.int32), "pool_final": ((B, W), torch.float32),
              "pool_sum": ((B, W), torch.float32), "pool_seq": ((B, W), torch.int32), "pool_cnt": ((B,), torch.int32),
              "pool_ins": ((B,), torch.int32), "res_tokens": ((B, W, cap), torch.int32), "res_logp": ((B, W, cap), torch.float32),
              "res_len": ((B, W), torch.int32), "res_final": ((B, W), torch.float32), "res_sum": ((B, W), torch.float32)}
    ptr = {}
    for name, (shape, dtype) in shapes.items():
        t = getattr(st, name)
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape, f"s2s_beam_select: {name} must be {dtype} {shape}"
        ptr["done_row" if name == "row_done" else name] = t.data_ptr()
    a = L.S2SBeamArgs(logits=pz, ldz=ldz, extra=px, ldx=ldx, inv_temp=float(inv_temp), dtype=dt(logits), B=B, W=W, V=V, cap=cap, eos=int(eos),
                      min_steps=int(min_steps), length_norm=1 if length_norm else 0, **ptr)
    L.check(L.lib().smx_s2s_beam_select(ctypes.byref(a), _stream()), "smx_s2s_beam_select")


# ---- CTC prefix scoring for the beam search (csrc/ctc_prefix.hip).  cs: a decoders.scorer.CTCPrefixState (x (B, T, V) fp32 CTC
# log-probabilities, enc_len (B) int32, state (2, R, T, 2) / psi (2, R) / extra (R, V) fp32, blank, eos, weight); st: the beam part of
# a Transformer.DecodeState, which the kernels only read.
def _ctc_prefix_args(cs, st, logits=None, inv_temp=1.0):
    B, W, cap = st.B, st.beam, st.cap
    R = B * W
    x = cs.x
    if not (x.is_cuda and cs.state.is_cuda):
        raise RuntimeError(NO_CPU)
    T, V = x.shape[1], x.shape[2]
    f32, i32 = torch.float32, torch.int32
    want = {"x": (cs.x, (B, T, V), f32), "enc_len": (cs.enc_len, (B,), i32), "state": (cs.state, (2, R, T, 2), f32),
            "psi": (cs.psi, (2, R), f32), "extra": (cs.extra, (R, V), f32), "score": (st.score, (R,), f32),
            "done": (st.done, (B,), torch.uint8), "n_tok": (st.n_tok, (B,), i32), "tokens": (st.tokens, (R, cap), i32),
            "anc": (st.anc, (R, cap), i32)}
    ptr = {}
    for name, (t, shape, dtype) in want.items():
        assert t.is_cuda and t.is_contiguous() and t.dtype == dtype and tuple(t.shape) == shape, f"ctc_prefix: {name} must be {dtype} {shape}"
        ptr[name] = t.data_ptr()
    a = L.CtcPrefixArgs(ldx=V, lde=V, inv_temp=float(inv_temp), weight=float(cs.weight), dtype=L.F32, B=B, W=W, V=V, T=T, cap=cap,
                        blank=int(cs.blank), eos=int(cs.eos), **ptr)
    if logits is not None:
        assert logits.is_cuda and tuple(logits.shape) == (R, V), f"ctc_prefix_score: logits must be (B W, V) = {(R, V)}"
        pz, a.ldz = _mat(logits)
        a.logits, a.dtype = pz, dt(logits)
    return a


def ctc_prefix_init(cs, st):
    """The prefix state of the empty hypothesis into slot 0 of every utterance, parity 0 (smx_ctc_prefix_init)."""
    L.check(L.lib().smx_ctc_prefix_init(ctypes.byref(_ctc_prefix_args(cs, st)), _stream()), "smx_ctc_prefix_init")


def ctc_prefix_score(cs, st, logits, inv_temp=1.0):
    """cs.extra (B W, V) = weight (ctc - lp) for the step the selection is about to take over logits (smx_ctc_prefix_score)."""
    tok = _pb(f"ctc_prefix_score (R {st.B * st.beam}, V {cs.x.shape[2]}, T {cs.x.shape[1]})", 4.0 * cs.x.numel() * st.beam)
    L.check(L.lib().smx_ctc_prefix_score(ctypes.byref(_ctc_prefix_args(cs, st, logits, inv_temp)), _stream()), "smx_ctc_prefix_score")
    _pe(tok)
    return cs.extra


def ctc_prefix_advance(cs, st):
    """The prefix state of every slot the selection just filled, from its parent's (smx_ctc_prefix_advance)."""
    L.check(L.lib().smx_ctc_prefix_advance(ctypes.byref(_ctc_prefix_args(cs, st)), _stream()), "smx_ctc_prefix_advance")


# ---- the language model's share of the scorer hook (csrc/lm_score.hip)
def lm_score(logits, extra, st, weight, inv_temp=1.0, accumulate=False):
    """extra (B W, V) fp32 (+)= weight * log_softmax(logits * inv_temp) over the LM's logits (B W, V) of the step the selection is about
    to take (smx_lm_score): written when accumulate is false, added to what smx_ctc_prefix_score wrote when it is true.  st: the beam
    part of a Transformer.DecodeState (score, done, n_tok), which the kernel only reads.  Rows that score nothing: include/smx.h."""
    if not (logits.is_cuda and extra.is_cuda):
        raise RuntimeError(NO_CPU)
    R, V = logits.shape
    B, W, cap = st.B, st.beam, st.cap
    assert R == B * W, f"lm_score: logits must have B W = {B * W} rows, got {R}"
    assert extra.dtype == torch.float32 and tuple(extra.shape) == (R, V), f"lm_score: extra must be float32 {(R, V)}"
    assert st.score.is_cuda and st.score.dtype == torch.float32 and st.score.is_contiguous() and st.score.shape == (R,)
    assert st.done.dtype == torch.uint8 and st.done.is_contiguous() and st.done.shape == (B,)
    assert st.n_tok.dtype == torch.int32 and st.n_tok.is_contiguous() and st.n_tok.shape == (B,)
    pz, ldz = _mat(logits)
    px, lde = _mat(extra)
    a = L.LmScoreArgs(logits=pz, ldz=ldz, extra=px, lde=lde, score=st.score.data_ptr(), done=st.done.data_ptr(), n_tok=st.n_tok.data_ptr(),
                      inv_temp=float(inv_temp), weight=float(weight), dtype=dt(logits), B=B, W=W, V=V, cap=cap, accumulate=1 if accumulate else 0)
    tok = _pb(f"lm_score {'bf16' if _es(logits) == 2 else 'f32'} (R {R}, V {V})" + (" acc" if accumulate else ""),
              R * V * (2 * _es(logits) + (8 if accumulate else 4)))
    L.check(L.lib().smx_lm_score(ctypes.byref(a), _stream()), "smx_lm_score")
    _pe(tok)
    return extra


# ---- transducer beam search (csrc/tbeam.hip).  st: a nnet.transducer.beam.TransducerBeamState - the weight images, the staging rows,
# the opaque state block, the counters and the result, all on the device and updated IN PLACE; nothing here synchronises with the host.
def tbeam_ok(dtype, H, J, V, W):
    return dtype in _DT and bool(L.lib().smx_tbeam_ok(_DT[dtype], H, J, V, W))


def tbeam_state_bytes(dtype, B, H, W, max_expansions, max_symbols, lm_layers=0, lm_H=0):
    return int(L.lib().smx_tbeam_state_bytes(_DT[dtype], B, H, W, max_expansions, max_symbols, lm_layers, lm_H))


def _tbeam_args(st, lm_logits=None):
    enc = st.enc
    if not enc.is_cuda:
        raise RuntimeError(NO_CPU)
    B, T, J = enc.shape
    H, V, W, nb, U, DT = st.H, st.V, st.W, st.nbest, st.U, enc.dtype
    f32, i32 = torch.float32, torch.int32
    want = {"WihT": (st.WihT, None, DT), "bias": (st.bias, (4 * H,), f32), "Whh": (st.Whh, (4 * H, H), DT), "Wproj": (st.Wproj, (J, H), DT),
            "Wlin": (st.Wlin, (V, J), DT), "cur_tok": (st.cur_tok, (B,), i32), "h_in": (st.h_in, (B, H), DT), "c_in": (st.c_in, (B, H), f32),
            "h_out": (st.h_out, (B, H), DT), "c_out": (st.c_out, (B, H), f32), "pdec": (st.pdec, (B, J), DT), "z": (st.z, (B, V), f32),
            "done": (st.done, (B,), torch.uint8), "overflow": (st.overflow, (B,), i32), "expansions": (st.expansions, (B,), i32),
            "frames": (st.frames, (B,), i32), "tokens": (st.tokens, (B, nb, U), i32), "out_len": (st.out_len, (B, nb), i32),
            "scores": (st.scores, (B, nb), f32), "sums": (st.sums, (B, nb), f32), "n_hyps": (st.n_hyps, (B,), i32)}
    if st.blin is not None:
        want["blin"] = (st.blin, (V,), f32)
    if st.lengths is not None:
        want["lengths"] = (st.lengths, (B,), i32)
    Lc, Hl = st.lm_L, st.lm_H
    if Lc:
        want.update({"lm_h_in": (st.lm_h_in, (Lc, B, Hl), DT), "lm_c_in": (st.lm_c_in, (Lc, B, Hl), f32),
                     "lm_h_out": (st.lm_h_out, (Lc, B, Hl), DT), "lm_c_out": (st.lm_c_out, (Lc, B, Hl), f32)})
    ptr = {}
    for name, (t, shape, dtype) in want.items():
        assert t.is_cuda and t.dtype == dtype and (shape is None or (t.is_contiguous() and tuple(t.shape) == shape)), \
            f"tbeam: {name} must be {dtype} {shape}"
        ptr[name] = t.data_ptr()
    assert st.WihT.shape == (V - 1, 4 * H) and st.WihT.stride(1) == 1 and enc.stride(2) == 1
    assert st.state.dtype == torch.uint8 and st.state.numel() >= tbeam_state_bytes(DT, B, H, W, st.E, U, Lc, Hl)
    a = L.TbeamArgs(enc=enc.data_ptr(), ld_b=enc.stride(0), ld_t=enc.stride(1), ldw=st.WihT.stride(0), state=st.state.data_ptr(),
                    lm_weight=float(st.lm_weight), state_beam=float(st.state_beam), expand_beam=float(st.expand_beam), dtype=_DT[DT], B=B, T=T,
                    H=H, J=J, V=V, W=W, nbest=nb, E=st.E, U=U, act=st.act, blank=st.blank, lm_L=Lc, lm_H=Hl, **ptr)
    if lm_logits is not None:
        assert Lc and lm_logits.is_cuda and lm_logits.dtype == DT and tuple(lm_logits.shape) == (B, V) and lm_logits.stride(1) == 1
        a.lm_logits, a.ld_lm = lm_logits.data_ptr(), lm_logits.stride(0)
    return a


def tbeam_init(st):
    """The start of a search (smx_tbeam_init): the hypothesis [blank] of every utterance, picked and staged; counters and result cleared."""
    L.check(L.lib().smx_tbeam_init(ctypes.byref(_tbeam_args(st)), _stream()), "smx_tbeam_init")


def tbeam_step(st):
    """The arithmetic of one expansion (smx_tbeam_step): LSTM step on cur_tok from h_in / c_in -> h_out / c_out, pdec, and the joint
    logits z (B, V) fp32 of every utterance's current frame.  Three launches."""
    L.check(L.lib().smx_tbeam_step(ctypes.byref(_tbeam_args(st)), _stream()), "smx_tbeam_step")


def tbeam_select(st, lm_logits=None):
    """The selection of one expansion (smx_tbeam_select) over st.z and, with an LM, its logits (B, V) for cur_tok.  One launch."""
    L.check(L.lib().smx_tbeam_select(ctypes.byref(_tbeam_args(st, lm_logits)), _stream()), "smx_tbeam_select")


# ---- the same search carried across streaming chunks.  st: a nnet.transducer.beam.TransducerBeamStreamState - st.enc
# holds ONE chunk (B, C, J), st.lengths the chunk's frames per slot, st.frames the frame inside the chunk, and two more device vectors:
# st.start (B) uint8 and st.stream_frames (B) int32, the frames closed over the whole stream.
def _tbeam_stream_vec(st, name, dtype):
    t = getattr(st, name)
    assert t.is_cuda and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == (st.enc.shape[0],), f"tbeam: {name} must be {dtype} (B,)"
    return t.data_ptr()


def tbeam_resume(st):
    """The start of a chunk (smx_tbeam_resume): slots with st.start set begin a new stream (smx_tbeam_init's work for that row), dead slots
    and slots without frames in this chunk are left as they were, the others are re-armed at the hypothesis staged at the pause."""
    L.check(L.lib().smx_tbeam_resume(ctypes.byref(_tbeam_args(st)), _tbeam_stream_vec(st, "start", torch.uint8),
                                     _tbeam_stream_vec(st, "stream_frames", torch.int32), _stream()), "smx_tbeam_resume")


def tbeam_select_stream(st, lm_logits=None):
    """smx_tbeam_select for a stream (smx_tbeam_select_stream): at a chunk's last frame the result is written AND the frame end is done,
    done[b] = 1 meaning paused.  One launch."""
    L.check(L.lib().smx_tbeam_select_stream(ctypes.byref(_tbeam_args(st, lm_logits)), _tbeam_stream_vec(st, "stream_frames", torch.int32),
                                            _stream()), "smx_tbeam_select_stream")
