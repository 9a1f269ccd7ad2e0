"""The GEMM route table shared by tests/test_gemm_routes_cpu.py and tests/test_gemm_routes_gpu.py (DESIGN.md "GEMM routes").

A case is plain data: name, dtype, layout, N, M, K, batch, splits, an alignment class, an epilogue family, the environment knobs it
needs and the plan smx_gemm_plan_query must report for it: (kernel, a_kc, b_kc, tile_n, tile_m, vec, lnf, gather).  The expected plan
is written down per ROUTE (the functions below name the route first and then list the shapes sent to it); a shape that lands elsewhere
is a wrong shape, never a reason to edit the route.

Operand geometry (`geometry`) is a pure function of the case, so that the CPU test can fabricate pointers of exactly the alignment
the GPU test's real views have:
  aligned - the view starts on a 16-byte boundary, ld = width rounded up to 8 elements + 8 (a multiple of 16 bytes);
  offset  - the view starts 8 elements into a wider row, ld = width + 8: still whole 16-byte items, so still the vector kernels;
  odd     - the view starts 1 element into the row and ld is odd: the element-guarded (non-vector) kernels.
Every matrix operand sits between `guard` rows before and after it (per batch), which the GPU test poisons."""
import collections

Case = collections.namedtuple("Case", "name dtype layout N M K batch splits align epi env plan")

ACT_NONE, ACT_GELU, ACT_SWISH, ACT_LEAKY, ACT_RELU = 0, 1, 2, 3, 4
KC = {"NT": (1, 1), "NN": (1, 0), "TN": (0, 0)}
C0_DIV = 50                      # group / period of the C0 rows: boundaries at 50, 100, 150 ... fall inside 64- and 128-row tiles


def plan(layout, tn, tm, vec, lnf=0):
    return (0,) + KC[layout] + (tn, tm, vec, lnf, 0)


DMA = (1, 0, 0, 128, 128, 1, 0, 0)

# ---- epilogue families ------------------------------------------------------------------------------------------------------------
# family -> fields.  out: "T" (the operand dtype), "F32", "ATOMIC".  z: "save" (written) | "grad" (SMX_EPI_ACT_GRAD: read).
# res: "T" | "F32" (SMX_IO_RES_F32).  drop: (p, seed).  drop_cols: "half" = the first M / 2 columns rounded down to 8.
_E = dict(bias=False, c0=None, c0_post=False, act=ACT_NONE, out="T", z=None, mask=False, res=None, alpha=1.0, drop=None, drop_cols=None,
          colsum=False, bias_batch=False, ln=None)


def _fam(**kw):
    d = dict(_E)
    d.update(kw)
    return d


FAMILIES = {
    "plain": _fam(),
    "bias_mask": _fam(bias=True, mask=True, alpha=0.5),
    "full_gelu": _fam(bias=True, act=ACT_GELU, z="save", mask=True, res="T", alpha=0.5),
    "full_swish": _fam(bias=True, act=ACT_SWISH, z="save", mask=True, res="T", alpha=0.5),
    "full_relu": _fam(bias=True, act=ACT_RELU, z="save", mask=True, res="T", alpha=0.5),
    "full_leaky": _fam(bias=True, act=ACT_LEAKY, z="save", mask=True, res="T", alpha=0.5),
    "c0_row": _fam(bias=True, c0="row"), "c0_group": _fam(bias=True, c0="group"), "c0_mod": _fam(bias=True, c0="mod"),
    "c0_row_post": _fam(bias=True, c0="row", c0_post=True, act=ACT_RELU, mask=True),
    "c0_group_post": _fam(bias=True, c0="group", c0_post=True, act=ACT_RELU, mask=True),
    "c0_mod_post": _fam(bias=True, c0="mod", c0_post=True, act=ACT_RELU, mask=True),
    "actgrad_gelu": _fam(act=ACT_GELU, z="grad", colsum=True, mask=True, drop=(0.2, 0x51A7E5), alpha=0.5),
    "actgrad_swish": _fam(act=ACT_SWISH, z="grad", colsum=True, mask=True, drop=(0.2, 0x51A7E5), alpha=0.5),
    "f32res": _fam(bias=True, out="F32", res="F32", alpha=0.5),
    "f32out": _fam(bias=True, out="F32"),
    "dropcols": _fam(bias=True, act=ACT_SWISH, drop=(0.25, 4242), drop_cols="half"),
    "bias_batch": _fam(bias=True, bias_batch=True, act=ACT_RELU),
    "atomic": _fam(out="ATOMIC"),
    # the five LayerNorm forms (+ the float32 LayerNorm-input variants of the backward: lnf 5 / 7)
    "ln_bwd": _fam(res="T", ln=dict(kind="bwd")),
    "ln_bwd_dx2": _fam(res="T", ln=dict(kind="bwd", dx2=True, mask2=True, alpha2=0.5, drop2=(0.25, 0x1234567))),
    "ln_bwd_ext": _fam(act=ACT_GELU, ln=dict(kind="bwd", dx2=True, alpha2=1.0, z2=True, lnf_act=ACT_SWISH)),
    "ln_bwd_x32": _fam(res="T", ln=dict(kind="bwd", x32=True)),
    "ln_bwd_ext_x32": _fam(act=ACT_SWISH, ln=dict(kind="bwd", dx2=True, mask2=True, alpha2=0.5, z2=True, lnf_act=ACT_NONE, x32=True)),
    "ln_fwd_bf16": _fam(bias=True, res="T", alpha=0.5, ln=dict(kind="fwd", lnf_act=ACT_SWISH)),
    "ln_fwd_f32": _fam(bias=True, out="F32", res="F32", alpha=0.5, mask=True, ln=dict(kind="fwd")),
    "ln_fwd_f32_y32": _fam(bias=True, out="F32", res="F32", alpha=0.5, drop=(0.25, 777), ln=dict(kind="fwd", y32=True)),
    "ln_fwd2": _fam(bias=True, out="F32", res="F32", alpha=0.5, ln=dict(kind="fwd", y32=True, pair=True)),
}
LNF_OF = {"ln_bwd": 1, "ln_bwd_dx2": 1, "ln_bwd_ext": 3, "ln_bwd_x32": 5, "ln_bwd_ext_x32": 7, "ln_fwd_bf16": 2, "ln_fwd_f32": 2,
          "ln_fwd_f32_y32": 2, "ln_fwd2": 2}


def fam(case):
    return FAMILIES[case.epi]


def drop_cols(case):
    f = fam(case)
    return (case.M // 2) // 8 * 8 if f["drop_cols"] == "half" else 0


def c0_rows(case):
    return {"row": case.N, "group": (case.N + C0_DIV - 1) // C0_DIV, "mod": C0_DIV}[fam(case)["c0"]]


# ---- operands ---------------------------------------------------------------------------------------------------------------------
Op = collections.namedtuple("Op", "name rows width dtype role batched dense")     # dtype: "T" | "f32" | "u8"; role: "r" | "w"


def operands(case):
    """Every tensor the call reads or writes.  Matrix operands of the output's shape (C, z, res) share one geometry: the kernel steps
    all three with the output's batch stride."""
    f, N, M, K = fam(case), case.N, case.M, case.K
    a = (K, N) if case.layout == "TN" else (N, K)
    b = (M, K) if case.layout == "NT" else (K, M)
    ops = [Op("A", a[0], a[1], "T", "r", True, False), Op("B", b[0], b[1], "T", "r", True, False),
           Op("C", N, M, "T" if f["out"] == "T" else "f32", "w", True, False)]
    if f["bias"]:
        ops.append(Op("bias", case.batch if f["bias_batch"] else 1, M, "f32", "r", False, False))
    if f["c0"]:
        ops.append(Op("c0", c0_rows(case), M, "f32", "r", False, False))
    if f["z"]:
        ops.append(Op("z", N, M, "T", "w" if f["z"] == "save" else "r", True, False))
    if f["mask"]:
        ops.append(Op("row_mask", 1, N, "u8", "r", False, True))
    if f["res"]:
        ops.append(Op("res", N, M, "f32" if f["res"] == "F32" else "T", "r", True, False))
    if f["colsum"]:
        ops.append(Op("colsum", 1, M, "f32", "w", False, True))
    ln = f["ln"]
    if ln and ln["kind"] == "bwd":
        tiles = (N + case.plan[3] - 1) // case.plan[3]
        ops += [Op("ln_x", N, M, "f32" if ln.get("x32") else "T", "r", False, False), Op("ln_stats", N, 2, "f32", "r", False, True),
                Op("ln_gamma", 1, M, "f32", "r", False, True), Op("ln_partial", 2 * tiles, M, "f32", "w", False, True)]
        if ln.get("dx2"):
            ops.append(Op("ln_dx2", N, M, "T", "w", False, False))
        if ln.get("mask2"):
            ops.append(Op("ln_mask2", 1, N, "u8", "r", False, True))
        if ln.get("z2"):
            ops.append(Op("z", N, M, "T", "r", True, False))
        if ln.get("lnf_act"):
            ops.append(Op("lnf_beta", 1, M, "f32", "r", False, True))
    if ln and ln["kind"] == "fwd":
        ops += [Op("lnf_gamma", 1, M, "f32", "r", False, True), Op("lnf_beta", 1, M, "f32", "r", False, True),
                Op("lnf_y", N, M, "f32" if ln.get("y32") else "T", "w", False, False), Op("lnf_stats", N, 2, "f32", "w", False, True)]
        if ln.get("pair"):
            ops += [Op("lnf2_gamma", 1, M, "f32", "r", False, True), Op("lnf2_beta", 1, M, "f32", "r", False, True),
                    Op("lnf2_y", N, M, "T", "w", False, False), Op("lnf2_stats", N, 2, "f32", "w", False, True)]
    return ops


Geo = collections.namedtuple("Geo", "coff ld guard bstride nbatch")     # all in elements / rows


def geometry(case, op):
    """Where the view of `op` sits in its buffer: buffer = nbatch x (guard + rows + guard) rows of ld elements, the view of batch i
    starts at element i * bstride + guard * ld + coff."""
    guard = case.plan[3] if op.rows == case.N else (4 if op.dense else 2)
    if op.dense:                                           # contiguous by contract (statistics, partial rows, [M] vectors, masks)
        coff, ld = 0, op.width
    elif case.align == "aligned":
        coff, ld = 0, (op.width + 7) // 8 * 8 + 8
    elif case.align == "offset":
        coff, ld = 8, op.width + 8
    else:
        coff, ld = 1, (op.width + 9) | 1
    nb = case.batch if op.batched else 1
    return Geo(coff, ld, guard, (op.rows + 2 * guard) * ld, nb)


def esize(case, op):
    return {"T": 2 if case.dtype == "bf16" else 4, "f32": 4, "u8": 1}[op.dtype]


def view_offset(case, op):
    g = geometry(case, op)
    return g.guard * g.ld + g.coff


def make_epilogue(case, ptr):
    """The smx_epilogue of the case; ptr(name) -> address of the operand's view (batch 0).  Used with fabricated addresses by the CPU
    test and with data_ptr()s by the GPU test: one builder, so the two cannot drift apart."""
    from summarymixing_amd import _lib as L
    f = fam(case)
    geo = {o.name: geometry(case, o) for o in operands(case)}
    e = L.Epilogue()
    e.alpha = f["alpha"]
    e.act = f["act"]
    e.out_mode = {"T": L.OUT_T, "F32": L.OUT_F32, "ATOMIC": L.OUT_ATOMIC_F32}[f["out"]]
    if f["bias"]:
        e.bias = ptr("bias")
        e.bias_batch_stride = geo["bias"].ld if f["bias_batch"] else 0
    if f["c0"]:
        e.c0, e.ldc0 = ptr("c0"), geo["c0"].ld
        e.c0_mode = {"row": L.C0_ROW, "group": L.C0_GROUP, "mod": L.C0_MOD}[f["c0"]]
        e.c0_div = C0_DIV
        if f["c0_post"]:
            e.flags |= L.EPI_C0_POST
    if f["z"]:
        e.z, e.ldz = ptr("z"), geo["z"].ld
        if f["z"] == "grad":
            e.flags |= L.EPI_ACT_GRAD
    if f["mask"]:
        e.row_mask = ptr("row_mask")
    if f["res"]:
        e.res, e.ldr = ptr("res"), geo["res"].ld
        if f["res"] == "F32":
            e.io_flags |= L.IO_RES_F32
    if f["drop"]:
        e.drop_p, e.drop_seed = f["drop"]
        e.drop_cols = drop_cols(case)
    if f["colsum"]:
        e.colsum = ptr("colsum")
        e.workspace = ptr("workspace")
    ln = f["ln"]
    if ln and ln["kind"] == "bwd":
        e.flags |= L.EPI_LN_BWD
        e.ln_x, e.ln_ldx = ptr("ln_x"), geo["ln_x"].ld
        e.ln_stats, e.ln_gamma, e.ln_partial = ptr("ln_stats"), ptr("ln_gamma"), ptr("ln_partial")
        if ln.get("x32"):
            e.io_flags |= L.IO_LNX_F32
        if ln.get("dx2"):
            e.ln_dx2, e.ln_lddx2, e.ln_alpha2 = ptr("ln_dx2"), geo["ln_dx2"].ld, ln["alpha2"]
            if ln.get("mask2"):
                e.ln_mask2 = ptr("ln_mask2")
            if ln.get("drop2"):
                e.ln_drop_p2, e.ln_drop_seed2 = ln["drop2"]
        if ln.get("z2"):
            e.z, e.ldz = ptr("z"), geo["z"].ld
        if ln.get("lnf_act"):
            e.lnf_beta, e.lnf_act = ptr("lnf_beta"), ln["lnf_act"]
    if ln and ln["kind"] == "fwd":
        e.flags |= L.EPI_LN_FWD
        e.lnf_gamma, e.lnf_beta, e.lnf_y, e.lnf_ldy = ptr("lnf_gamma"), ptr("lnf_beta"), ptr("lnf_y"), geo["lnf_y"].ld
        e.lnf_stats, e.lnf_eps, e.lnf_act = ptr("lnf_stats"), 1e-5, ln.get("lnf_act", ACT_NONE)
        if ln.get("y32"):
            e.io_flags |= L.IO_LNFY_F32
        if ln.get("pair"):
            e.lnf2_gamma, e.lnf2_beta, e.lnf2_y, e.lnf2_ldy = ptr("lnf2_gamma"), ptr("lnf2_beta"), ptr("lnf2_y"), geo["lnf2_y"].ld
            e.lnf2_stats, e.lnf2_eps = ptr("lnf2_stats"), 1e-5
    return e


def gemm_args(case, ptr):
    """(layout, dtype, A, lda, sA, B, ldb, sB, C, ldc, sC, N, M, K, batch, splits) of smx_gemm / smx_gemm_plan_query."""
    from summarymixing_amd import _lib as L
    o = {x.name: x for x in operands(case)}
    ga, gb, gc = geometry(case, o["A"]), geometry(case, o["B"]), geometry(case, o["C"])
    one = case.batch == 1
    return ({"NT": L.GEMM_NT, "NN": L.GEMM_NN, "TN": L.GEMM_TN}[case.layout], L.BF16 if case.dtype == "bf16" else L.F32,
            ptr("A"), ga.ld, 0 if one else ga.bstride, ptr("B"), gb.ld, 0 if one else gb.bstride, ptr("C"), gc.ld,
            0 if one else gc.bstride, case.N, case.M, case.K, case.batch, case.splits)


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def _mk(out, route, dtype, layout, shape, align, epi, pl, env=None, batch=1, splits=1):
    N, M, K = shape
    name = f"{route}-{dtype}-{layout}-{N}x{M}x{K}" + (f"-b{batch}" if batch > 1 else "") + (f"-s{splits}" if splits > 1 else "") + f"-{align}-{epi}"
    out.append(Case(name, dtype, layout, N, M, K, batch, splits, align, epi, dict(env or {}), pl))


GENERAL = ("full_gelu", "full_swish", "full_relu", "full_leaky", "c0_row", "c0_group", "c0_mod", "c0_row_post", "c0_group_post", "c0_mod_post",
           "actgrad_gelu", "f32out", "dropcols")


def _tile64(t):
    """64 x 64: fewer than 256 tiles of 128.  Vector and element-guarded kernels, both dtypes, all three layouts."""
    vshape = {("bf16", "NT"): (129, 72, 128), ("bf16", "NN"): (129, 72, 128), ("bf16", "TN"): (136, 72, 100),
              ("f32", "NT"): (130, 68, 36), ("f32", "NN"): (130, 68, 36), ("f32", "TN"): (132, 68, 37)}
    for (dt, lay), shp in vshape.items():
        _mk(t, "t64", dt, lay, shp, "aligned", "plain", plan(lay, 64, 64, 1))
        _mk(t, "t64", dt, lay, shp, "odd", "plain", plan(lay, 64, 64, 0))
        _mk(t, "t64", dt, lay, (37, 19, 23), "aligned", "plain", plan(lay, 64, 64, 0))      # ragged: no whole vectors whatever the alignment
    for dt in ("bf16", "f32"):
        shp = vshape[(dt, "NT")]
        _mk(t, "t64", dt, "NT", shp, "offset", "plain", plan("NT", 64, 64, 1))
        _mk(t, "t64", dt, "NN", shp, "offset", "full_swish", plan("NN", 64, 64, 1))
        for epi in GENERAL:
            lay = "NN" if epi.startswith("actgrad") else "NT"
            _mk(t, "t64", dt, lay, shp, "aligned", epi, plan(lay, 64, 64, 1))
            _mk(t, "t64", dt, lay, shp, "odd", epi, plan(lay, 64, 64, 0))
        _mk(t, "t64", dt, "NN", shp, "aligned", "bias_batch", plan("NN", 64, 64, 1), batch=3)
        _mk(t, "t64", dt, "NN", shp, "odd", "bias_batch", plan("NN", 64, 64, 0), batch=3)
    _mk(t, "t64", "bf16", "NT", vshape[("bf16", "NT")], "aligned", "f32res", plan("NT", 64, 64, 1))
    # (no odd sibling: SMX_IO_RES_F32 requires a 16-byte aligned residual; `f32out` is the float32 output of the odd class)
    _mk(t, "t64", "bf16", "NT", (37, 19, 23), "aligned", "full_gelu", plan("NT", 64, 64, 0))
    _mk(t, "t64", "f32", "NN", (37, 19, 23), "odd", "c0_group_post", plan("NN", 64, 64, 0))


def _tile128(t):
    """128 x 128: at least 256 tiles (batch multiplies), M not a multiple of 256."""
    for dt in ("bf16", "f32"):
        for lay in ("NT", "NN", "TN"):
            shp = (136, 136, 64) if lay == "TN" else (129, 136, 64)
            _mk(t, "t128", dt, lay, shp, "aligned", "plain", plan(lay, 128, 128, 1), batch=64)
            _mk(t, "t128", dt, lay, shp, "odd", "plain", plan(lay, 128, 128, 0), batch=64)
        _mk(t, "t128", dt, "NT", (129, 136, 64), "aligned", "bias_batch", plan("NT", 128, 128, 1), batch=64)
        _mk(t, "t128", dt, "NT", (129, 136, 64), "odd", "bias_batch", plan("NT", 128, 128, 0), batch=64)
        _mk(t, "t128", dt, "NN", (129, 136, 64), "offset", "full_swish", plan("NN", 128, 128, 1), batch=64)
    _mk(t, "t128", "bf16", "NT", (129, 136, 40), "aligned", "full_gelu", plan("NT", 128, 128, 0), batch=64)      # K % 64 != 0: no buffer-load stages
    # the batch == 1 epilogues (C0 rows, act-grad + column sums, ...) need 16 x 16 tiles of their own
    big = (1921, 1928, 64)
    for epi in GENERAL + ("f32res",):
        lay = "NN" if epi.startswith("actgrad") else "NT"
        _mk(t, "t128", "bf16", lay, big, "aligned", epi, plan(lay, 128, 128, 1))
    for epi in ("full_swish", "c0_group", "c0_mod_post", "actgrad_swish", "dropcols", "f32out"):
        lay = "NN" if epi.startswith("actgrad") else "NT"
        _mk(t, "t128", "bf16", lay, big, "odd", epi, plan(lay, 128, 128, 0))
    for epi in ("full_gelu", "c0_group_post", "actgrad_gelu"):
        lay = "NN" if epi.startswith("actgrad") else "NT"
        _mk(t, "t128", "f32", lay, big, "aligned", epi, plan(lay, 128, 128, 1))
        _mk(t, "t128", "f32", lay, big, "odd", epi, plan(lay, 128, 128, 0))


def _wide(t):
    """128 x 256: M == 256 with at least 256 tiles, or K >= 2048 with M == 512."""
    for dt in ("bf16", "f32"):
        for lay in ("NT", "NN"):
            _mk(t, "wide", dt, lay, (129, 256, 64), "aligned", "plain", plan(lay, 128, 256, 1), batch=128)
            _mk(t, "wide", dt, lay, (129, 256, 64), "odd", "plain", plan(lay, 128, 256, 0), batch=128)
    _mk(t, "wide", "bf16", "TN", (136, 256, 64), "aligned", "plain", plan("TN", 128, 256, 1), batch=128)
    _mk(t, "wide", "bf16", "TN", (136, 256, 64), "odd", "plain", plan("TN", 128, 256, 0), batch=128)
    for epi in ("full_gelu", "full_swish", "bias_batch", "f32out"):
        _mk(t, "wide", "bf16", "NT", (129, 256, 64), "aligned", epi, plan("NT", 128, 256, 1), batch=128)
    _mk(t, "wide", "bf16", "NT", (129, 256, 64), "odd", "full_relu", plan("NT", 128, 256, 0), batch=128)
    _mk(t, "wide", "bf16", "NT", (129, 256, 64), "offset", "full_leaky", plan("NT", 128, 256, 1), batch=128)
    # batch == 1 forms: 256 row tiles of 128
    for epi in ("actgrad_gelu", "c0_group", "f32res"):
        lay = "NN" if epi.startswith("actgrad") else "NT"
        _mk(t, "wide", "bf16", lay, (32641, 256, 64), "aligned", epi, plan(lay, 128, 256, 1))
    _mk(t, "wide", "bf16", "NN", (32641, 256, 64), "odd", "actgrad_swish", plan("NN", 128, 256, 0))
    # the second clause: a long reduction into M == 512 (batched, so the 256 x 256 tile is not eligible)
    _mk(t, "wide", "bf16", "NT", (129, 512, 2048), "aligned", "full_swish", plan("NT", 128, 256, 1), batch=64)
    _mk(t, "wide", "bf16", "NN", (129, 512, 2048), "odd", "plain", plan("NN", 128, 256, 0), batch=64)


def _t256(t):
    """256 x 256 (one workgroup per CU): by default K >= 2048, M % 256 == 0, an epilogue without element-wise side inputs writing dtype
    T and at least 200 tiles; SMX_T256=2 every eligible shape; SMX_T256=3 the M == 512 shapes on the plain 128 x 512 tile."""
    _mk(t, "t256", "bf16", "NT", (25345, 512, 2048), "aligned", "bias_mask", plan("NT", 256, 256, 1))
    _mk(t, "t256", "bf16", "NN", (25345, 512, 2048), "aligned", "plain", plan("NN", 256, 256, 1))
    epis = ("plain", "full_swish", "c0_group", "actgrad_gelu", "f32res", "dropcols")
    for i, shp in enumerate(((257, 256, 128), (300, 512, 128), (513, 768, 192))):
        for j, epi in enumerate(epis):
            lay = "NN" if epi.startswith("actgrad") or (i + j) % 2 else "NT"
            _mk(t, "t256", "bf16", lay, shp, "aligned", epi, plan(lay, 256, 256, 1), env={"SMX_T256": "2"})
    for j, epi in enumerate(epis + ("full_gelu", "c0_mod_post")):
        lay = "NN" if epi.startswith("actgrad") or j % 2 else "NT"
        _mk(t, "row512", "bf16", lay, (300, 512, 128), "aligned", epi, plan(lay, 128, 512, 1), env={"SMX_T256": "3"})
    _mk(t, "t256", "bf16", "NT", (513, 768, 192), "aligned", "full_relu", plan("NT", 256, 256, 1), env={"SMX_T256": "3"})


def _dma(t):
    """gemm_tn_dma_kernel: bf16 TN, N and M multiples of 128, K of 64, at least 256 tiles, no element-wise side input."""
    for epi in ("plain", "bias_mask", "bias_batch", "f32out", "dropcols"):
        _mk(t, "dma", "bf16", "TN", (256, 256, 192), "aligned", epi, DMA, batch=64)
    _mk(t, "dma", "bf16", "TN", (256, 256, 192), "offset", "plain", DMA, batch=64)
    # the element-guarded sibling of the same shape: register-staged, 2 x 2 x 64 tiles of 128 (only 128 of the 128 x 256 tile: not wide)
    _mk(t, "dma", "bf16", "TN", (256, 256, 192), "odd", "plain", plan("TN", 128, 128, 0), batch=64)


LN_FORMS = ("ln_bwd", "ln_bwd_dx2", "ln_bwd_ext", "ln_bwd_x32", "ln_bwd_ext_x32", "ln_fwd_bf16", "ln_fwd_f32", "ln_fwd_f32_y32", "ln_fwd2")


def _ln(t):
    """LayerNorm-fused row-complete tiles: 64 x 256 (default below ~37 000 frames), 128 x 256 (default above; SMX_LN_TILE64=0), 128 x 512."""
    for i, epi in enumerate(LN_FORMS):
        lay = "NN" if epi.startswith("ln_bwd") else "NT"   # (the dgrad / forward layouts of the product; every other form flipped)
        if i in (1, 3, 6, 8):
            lay = "NT" if lay == "NN" else "NN"
        lnf = LNF_OF[epi]
        for N, K in ((128, 192), (200, 64)):
            _mk(t, "ln64", "bf16", lay, (N, 256, K), "aligned", epi, plan(lay, 64, 256, 1, lnf))
        for N, K in ((128, 192), (129, 64)):
            _mk(t, "ln128", "bf16", lay, (N, 256, K), "aligned", epi, plan(lay, 128, 256, 1, lnf), env={"SMX_LN_TILE64": "0"})
        for N, K in ((128, 192), (200, 64)):
            _mk(t, "ln512", "bf16", lay, (N, 512, K), "aligned", epi, plan(lay, 128, 512, 1, lnf))
    # the other weight layout of the two commonest forms, and the default rule's 128-row tile
    _mk(t, "ln64", "bf16", "NT", (200, 256, 64), "aligned", "ln_bwd", plan("NT", 64, 256, 1, 1))
    _mk(t, "ln512", "bf16", "NN", (200, 512, 64), "offset", "ln_fwd_bf16", plan("NN", 128, 512, 1, 2))
    _mk(t, "ln128", "bf16", "NN", (32769, 256, 64), "aligned", "ln_bwd", plan("NN", 128, 256, 1, 1))
    _mk(t, "ln128", "bf16", "NT", (32769, 256, 64), "aligned", "ln_fwd_f32", plan("NT", 128, 256, 1, 2))


def _atomic(t):
    """Atomic split-K (SMX_OUT_ATOMIC_F32, splits = 3) on the 64 and 128 tiles: a last split shorter than kchunk, and a K whose
    effective split count is below the requested one.  The atomic output is never 16-byte staged (gemm_impl: epi_lds is false for
    SMX_OUT_ATOMIC_F32 and the vector kernels need it), so every one of these is the element-guarded kernel whatever the alignment."""
    for dt, ks in (("bf16", (320, 200)), ("f32", (150, 100))):         # kchunk 128 | 64: 3 splits (last 64 | 22), then 2 splits
        for K in ks:
            _mk(t, "atomic", dt, "TN", (136, 72, K), "aligned", "atomic", plan("TN", 64, 64, 0), splits=3)
            _mk(t, "atomic", dt, "NT" if dt == "f32" else "TN", (37, 19, K), "odd", "atomic", plan("NT" if dt == "f32" else "TN", 64, 64, 0), splits=3)
    _mk(t, "atomic", "bf16", "TN", (136, 136, 320), "aligned", "atomic", plan("TN", 128, 128, 0), batch=22, splits=3)
    _mk(t, "atomic", "bf16", "TN", (136, 136, 200), "odd", "atomic", plan("TN", 128, 128, 0), batch=32, splits=3)
    _mk(t, "atomic", "f32", "NN", (129, 136, 150), "aligned", "atomic", plan("NN", 128, 128, 0), batch=22, splits=3)


def table():
    t = []
    for part in (_tile64, _tile128, _wide, _t256, _dma, _ln, _atomic):
        part(t)
    names = [c.name for c in t]
    assert len(set(names)) == len(names), [n for n in names if names.count(n) > 1]
    return t


CASES = table()

# every `plan_only(` launch site reachable from smx_gemm, as (kernel, tile_n, tile_m, lnf, vec)
LAUNCH_SITES = (
    {(0, 64, 64, 0, 0), (0, 64, 64, 0, 1), (0, 128, 128, 0, 0), (0, 128, 128, 0, 1), (0, 128, 256, 0, 0), (0, 128, 256, 0, 1),      # launch_tile
     (0, 256, 256, 0, 1), (1, 128, 128, 0, 1)}                                                                                # 256 x 256; LDS-DMA TN
    | {(0, 64, 256, l, 1) for l in (1, 2, 3, 5, 7)} | {(0, 128, 256, l, 1) for l in (1, 2, 3, 5, 7)}                           # gemm_ln256r64 / gemm_ln256
    | {(0, 128, 512, l, 1) for l in (0, 1, 2, 3, 5, 7)})                                                                      # gemm_ln512


def env_key(case):
    return tuple(sorted(case.env.items()))


def env_groups():
    groups = collections.OrderedDict()
    for c in CASES:
        groups.setdefault(env_key(c), []).append(c)
    return groups
