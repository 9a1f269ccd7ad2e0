"""The bits and the launches of the attention sublayer, pinned: nnet.attention.MultiheadAttention on its three projection plans,
TransformerDecoderLayer / TransformerDecoder (self- and cross-attention with the residual, the dropout sites and the memory gradient
in the GEMM epilogues) and, for the one-input closure node, nnet.linear.Linear + SummaryMixing through functional.block.  Per case
tests/golden/attention_sublayer_bits.json holds the SHA-256 of the raw bytes of every output, every input gradient and every
parameter gradient, and the ordered list of launches: pass-through spies on the launch wrappers of summarymixing_amd.ops note each
call - tensors by dtype, shape, leading dimension and storage offset (tests/_util.describe), never by address - and then make it.
The float64 tests of these modules allow a tolerance and would not see a launch added, dropped, reordered or aimed at another view,
nor a dropout seed drawn at another place; this one does.  It uses the public modules only, so it runs unchanged on a tree whose host
orchestration is organised differently: the fixture was written before MultiheadAttention and the decoder layer shared one sublayer.

Inputs and parameters are integer patterns (tests/_util.pattern, exact in bf16), no random generator; the dropout cases fix
torch.manual_seed and the library's seed counter.  Shapes: B = 2, L = U = 17 (a full 16-row tile plus one row), S = 65 (a 64-key tile
plus one key), (d, H) = (256, 4) - the panel / LayerNorm-fused Linear routes - and (512, 1), the recipes' decoder, f32 and bf16.
`python tests/test_attention_sublayer_bits_gpu.py --write <path>` writes the fixture."""
import ctypes
import hashlib
import json
import os
import sys

import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))      # (for --write: run as a script)
from tests._util import describe, pattern  # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attention_sublayer_bits.json")
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
WIDTHS = {"d256h4": (256, 4), "d512h1": (512, 1)}
B, LQ, S, D_FFN = 2, 17, 65, 256
SPIED = ("gemm", "gemm_panel", "gemm_panel_slabs", "slab_epilogue", "wgrad", "wgrad_partial", "wgrad_group", "wgrad_group_direct",
         "reduce_jobs", "layernorm_fwd", "layernorm_bwd", "attention_fwd", "attention_bwd", "attention_weights", "cast", "dropout",
         "axpby", "act_mask_bwd", "new_dropout_seed")


class Spies:
    """Pass-through recorders on summarymixing_amd.ops: `with Spies() as launches` -> one string per call, in order.  ops.epilogue
    is wrapped as well, only to describe the epilogue a GEMM is handed by the arguments it was built from (the struct holds
    addresses)."""

    def __enter__(self):
        from summarymixing_amd import ops
        self.ops, self.saved, self.launches, self.epis = ops, {}, [], {}

        def fmt(v):
            if isinstance(v, torch.Tensor) and v.dtype == torch.uint8 and v.dim() == 1:
                return "u8[workspace]"                   # (a persistent per-parameter workspace: its size remembers earlier, larger uses)
            if isinstance(v, (ctypes.Structure, ctypes.Array)):
                return self.epis[id(v)][1] if id(v) in self.epis else type(v).__name__
            if isinstance(v, (tuple, list)):
                return "(" + ",".join(fmt(x) for x in v) + ")"
            if hasattr(v, "t") and isinstance(v.t, torch.Tensor):
                return f"{type(v).__name__}({describe(v.t)})"                # (ops.Slabs: split-K partial products)
            return describe(v)

        def spy(name, fn):
            def f(*a, **k):
                got = fn(*a, **k)
                line = " ".join([name] + [fmt(x) for x in a] + [f"{n}={fmt(x)}" for n, x in sorted(k.items())])
                self.launches.append(line + (f" -> {got}" if name == "new_dropout_seed" else ""))
                return got
            return f

        def epilogue(**kw):
            e = self.saved["epilogue"](**kw)
            self.epis[id(e)] = (e, "{" + ",".join(f"{k}={fmt(v)}" for k, v in sorted(kw.items()) if v is not None) + "}")   # (e is held: its id stays its own)
            return e
        for name in SPIED + ("epilogue",):
            self.saved[name] = getattr(ops, name)
            setattr(ops, name, epilogue if name == "epilogue" else spy(name, self.saved[name]))
        return self.launches

    def __exit__(self, *exc):
        for name, fn in self.saved.items():
            setattr(self.ops, name, fn)


def _digest(t):
    if t is None:
        return "none"
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _fill(module):
    """Every parameter from a pattern of its own (exact in bf16); LayerNorm weights around 1."""
    with torch.no_grad():
        for n, (name, p) in enumerate(module.named_parameters()):
            if p.dim() == 1:
                v = pattern(1, p.shape[0], (0, 7 + 2 * (n % 5)), 31, 8, -3, 2).view(-1) + (1.0 if name.endswith("norm.weight") else 0.0)
            else:
                v = pattern(p.shape[0], p.numel() // p.shape[0], (13 + 2 * (n % 7), 29), 53, 16, -6, 3).view(p.shape)
            p.copy_(v.float())
    return module.cuda()


def _act(rows, d, dtype, k, grad=True):
    """(B, rows, d) activations: pattern number k, within +-2."""
    x = pattern(B * rows, d, (37 + 4 * k, 11 + 2 * k), 61, 16, -2, 3).view(B, rows, d).to(dtype).cuda()
    return x.requires_grad_(grad)


def _cot(rows, d, dtype):
    return pattern(B * rows, d, (3, 5), 13, 8, -2, 3).view(B, rows, d).to(dtype).cuda()


def _pads():
    """Key-padding masks (B, LQ) and (B, S): utterance 1 padded at the tail, never position 0."""
    tpad = torch.zeros(B, LQ, dtype=torch.bool)
    mpad = torch.zeros(B, S, dtype=torch.bool)
    tpad[1, LQ - 3:] = True
    mpad[1, S // 2:] = True
    return tpad.cuda(), mpad.cuda()


class _Seeded:
    """torch.manual_seed(k) and the library's seed counter at a fixed value; the counter is put back (it is global)."""

    def __init__(self, k):
        self.k = k

    def __enter__(self):
        from summarymixing_amd import ops
        self.ops, self.saved = ops, ops._drop_state["counter"]
        torch.manual_seed(self.k)
        ops._drop_state["counter"] = 9000

    def __exit__(self, *exc):
        self.ops._drop_state["counter"] = self.saved


def _finish(outs, cot, inputs, module):
    """Backward of sum(out * cot) where anything needs it; -> the labelled tensors of the case."""
    got = {f"out{i}": o for i, o in enumerate(outs)}
    if outs[0].requires_grad:
        outs[0].backward(cot)
    for name, t in inputs.items():
        got["d " + name] = t.grad
    for name, p in module.named_parameters():
        got["d " + name] = p.grad
    return got


def _mha(dtype, d, H, plan, bias=True, grads=(True, True, True), mask=False, causal=False, weights=True, p=0.0, no_grad=False,
         strided=False):
    from summarymixing_amd.nnet.attention import MultiheadAttention
    m = _fill(MultiheadAttention(H, d, dropout=p, bias=bias)).train(p > 0.0)
    if strided:                                          # a (B, L, d) view of an (L, B, d) tensor: its rows are copied
        q = pattern(B * LQ, d, (37, 11), 61, 16, -2, 3).view(LQ, B, d).to(dtype).cuda().requires_grad_(grads[0])
        inputs = {"query": q}
        q = q.transpose(0, 1)
    else:
        q = _act(LQ, d, dtype, 0, grads[0])
        inputs = {"query": q}
    if plan == "self":
        k = v = q
    elif plan == "kv":
        k = v = inputs["key"] = _act(S, d, dtype, 1, grads[1])
    else:
        k, v = inputs["key"], inputs["value"] = _act(S, d, dtype, 1, grads[1]), _act(S, d, dtype, 2, grads[2])
    Sk = k.shape[1]
    kw = {"causal": causal, "return_attn_weights": weights}
    if mask:
        i, j = torch.arange(LQ).view(-1, 1), torch.arange(Sk).view(1, -1)
        kw["attn_mask"] = ((3 * i + 5 * j) % 7 == 0).cuda()                  # (every row keeps most of its keys)
        kw["key_padding_mask"] = _pads()[0 if plan == "self" else 1]
    with _Seeded(11), torch.set_grad_enabled(not no_grad):
        out = m(q, k, v, **kw)
        return _finish(out if weights else (out,), _cot(LQ, d, dtype), inputs, m)


def _layer(dtype, d, H, pre, train, mem_grad, mask, pads, no_grad=False):
    from summarymixing_amd.lobes.models.transformer.Transformer import LOOKAHEAD, TransformerDecoderLayer, get_lookahead_mask
    m = _fill(TransformerDecoderLayer(D_FFN, H, d, dropout=0.1 if train else 0.0, activation=nn.GELU, normalize_before=pre)).train(train)
    tgt, mem = _act(LQ, d, dtype, 0), _act(S, d, dtype, 1, mem_grad)
    tpad, mpad = _pads() if pads else (None, None)
    tgt_mask = {"look": LOOKAHEAD, "dense": get_lookahead_mask(tgt), "none": None}[mask]
    with _Seeded(12), torch.set_grad_enabled(not no_grad):
        outs = m(tgt, mem, tgt_mask=tgt_mask, tgt_key_padding_mask=tpad, memory_key_padding_mask=mpad)
        return _finish(outs, _cot(LQ, d, dtype), {"tgt": tgt, "memory": mem}, m)


def _decoder(dtype, d, H, pre, weights):
    from summarymixing_amd.lobes.models.transformer.Transformer import LOOKAHEAD, TransformerDecoder
    m = _fill(TransformerDecoder(2, H, D_FFN, d, dropout=0.1, activation=nn.GELU, normalize_before=pre, causal=True)).train()
    tgt, mem = _act(LQ, d, dtype, 0), _act(S, d, dtype, 1)
    tpad, mpad = _pads()
    with _Seeded(13):
        out, sa, ca = m(tgt, mem, tgt_mask=LOOKAHEAD, tgt_key_padding_mask=tpad, memory_key_padding_mask=mpad, _weights=weights)
        assert [w is None for w in sa + ca] == {"none": [True] * 4, "last_cross": [True, True, True, False], "all": [False] * 4}[weights]
        return _finish([out] + [w for w in sa + ca if w is not None], _cot(LQ, d, dtype), {"tgt": tgt, "memory": mem}, m)


def _block(dtype, x_grad):
    """Linear -> SummaryMixing, each one functional.block: the closure node with one activation in."""
    from summarymixing_amd.nnet.linear import Linear
    from summarymixing_amd.nnet.summary_mixing import SummaryMixing
    d = 64
    m = _fill(nn.Sequential(Linear(d, input_size=d), SummaryMixing(d, 1, [d], d, [d], d, global_dropout=0.0, mode="SummaryMixing")))
    x = _act(LQ, d, dtype, 0, x_grad)
    return _finish((m(x),), _cot(LQ, d, dtype), {"x": x}, m)


def _cases():
    cases = {}
    for dn, dtype in DTYPES.items():
        for wn, (d, H) in WIDTHS.items():
            a = (dtype, d, H)
            for name, kw in {
                    "self": dict(plan="self"), "self-noweights": dict(plan="self", weights=False), "self-causal": dict(plan="self", causal=True),
                    "self-mask-pad": dict(plan="self", mask=True), "self-dropout": dict(plan="self", p=0.1),
                    "self-no_grad": dict(plan="self", no_grad=True), "self-input-nograd": dict(plan="self", grads=(False,) * 3),
                    "kv": dict(plan="kv", weights=False), "kv-weights": dict(plan="kv"), "kv-nobias": dict(plan="kv", bias=False),
                    "kv-query-nograd": dict(plan="kv", grads=(False, True, True), weights=False),
                    "kv-memory-nograd": dict(plan="kv", grads=(True, False, False), weights=False),
                    "kv-mask-pad": dict(plan="kv", mask=True), "kv-dropout": dict(plan="kv", p=0.1), "kv-no_grad": dict(plan="kv", no_grad=True),
                    "kv-strided-query": dict(plan="kv", strided=True, weights=False),
                    "general": dict(plan="general"), "general-nobias": dict(plan="general", bias=False, weights=False),
                    "general-key-grad-only": dict(plan="general", grads=(True, True, False)),
                    "general-query-nograd": dict(plan="general", grads=(False, True, True), weights=False),
                    "general-dropout": dict(plan="general", p=0.1, weights=False)}.items():
                cases[f"mha-{name}-{wn}-{dn}"] = (_mha, a, kw)
            for pre, train, mem_grad, mask, pads in ((True, False, True, "look", True), (False, False, True, "look", True),
                                                     (True, True, True, "look", True), (False, True, True, "look", True),
                                                     (True, True, False, "dense", True), (False, True, False, "dense", True),
                                                     (True, False, False, "dense", False), (False, False, True, "none", False)):
                name = f"{'pre' if pre else 'post'}-{'train' if train else 'eval'}-{'dmem' if mem_grad else 'nodmem'}-{mask}-{'pads' if pads else 'nopads'}"
                cases[f"layer-{name}-{wn}-{dn}"] = (_layer, a, dict(pre=pre, train=train, mem_grad=mem_grad, mask=mask, pads=pads))
            cases[f"layer-pre-no_grad-{wn}-{dn}"] = (_layer, a, dict(pre=True, train=False, mem_grad=True, mask="look", pads=True, no_grad=True))
            for pre, weights in ((True, "none"), (True, "last_cross"), (True, "all"), (False, "last_cross")):
                cases[f"decoder-{'pre' if pre else 'post'}-{weights}-{wn}-{dn}"] = (_decoder, a, dict(pre=pre, weights=weights))
        for x_grad in (True, False):
            cases[f"block-linear-summarymixing-{'dx' if x_grad else 'nodx'}-{dn}"] = (_block, (dtype, x_grad), {})
    return cases


CASES = _cases()


def _run(name):
    """-> ({label: digest}, [launch, ...]) of one case."""
    from summarymixing_amd import functional as F
    fn, args, kw = CASES[name]
    F._evict_workspaces()                                # (no workspace of an earlier case at a re-used gradient address, no eviction in mid-case)
    with Spies() as launches:
        got = fn(*args, **kw)
        torch.cuda.synchronize()
    for label, t in got.items():
        assert t is None or bool(torch.isfinite(t.float()).all()), f"{name}: {label} is not finite"
    return {label: _digest(t) for label, t in got.items()}, launches


def _write(path):
    table, cases = {}, {}
    for name in sorted(CASES):
        bits, launches = _run(name)
        cases[name] = {"bits": bits, "launches": [table.setdefault(line, len(table)) for line in launches]}
    with open(path, "w") as f:
        json.dump({"launch_table": list(table), "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"wrote {len(cases)} cases, {len(table)} distinct launches to {path}")


@pytest.fixture(scope="module")
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.mark.parametrize("name", sorted(CASES))
def test_bits_and_launches_equal_the_fixture(name, golden):
    (bits, launches), want = _run(name), golden["cases"][name]
    want_launches = [golden["launch_table"][i] for i in want["launches"]]
    for i, (g, w_) in enumerate(zip(launches, want_launches)):
        assert g == w_, f"{name}: launch {i} differs from the fixture"
    assert len(launches) == len(want_launches), f"{name}: {len(launches)} launches, the fixture has {len(want_launches)}"
    assert sorted(bits) == sorted(want["bits"]), f"{name}: the tensors of the case differ from the fixture's"
    for label, g in bits.items():
        assert g == want["bits"][label], f"{name}: the bits of `{label}` differ from the fixture"


def test_fixture_has_exactly_these_cases(golden):
    assert sorted(golden["cases"]) == sorted(CASES)


def test_fixture_sees_the_paths_it_is_there_for(golden):
    """The cases must differ where the code under test branches, or the fixture would pin nothing: the three projection plans launch
    1 / 2 / 3 in-projection GEMMs; a skipped dgrad is a launch less; dropout changes the bits; f32 and bf16 round differently."""
    def lines(name):
        return [golden["launch_table"][i] for i in golden["cases"][name]["launches"]]

    def count(name, what):
        return sum(line.startswith(what + " ") for line in lines(name))
    for tail in ("d256h4-f32", "d512h1-bf16"):
        assert count(f"mha-self-{tail}", "attention_fwd") == count(f"mha-self-{tail}", "attention_bwd") == 1
        assert count(f"mha-self-{tail}", "attention_weights") == 1 and count(f"mha-self-noweights-{tail}", "attention_weights") == 0
        n = [len(lines(f"mha-{plan}-{tail}")) for plan in ("self-noweights", "kv", "general-nobias")]
        assert n[0] < n[1] < n[2], n
        assert len(lines(f"mha-kv-query-nograd-{tail}")) < len(lines(f"mha-kv-{tail}"))
        assert len(lines(f"layer-pre-train-nodmem-dense-pads-{tail}")) < len(lines(f"layer-pre-train-dmem-look-pads-{tail}"))
        assert count(f"mha-self-dropout-{tail}", "new_dropout_seed") == 1 and count(f"mha-self-{tail}", "new_dropout_seed") == 0
        assert count(f"layer-pre-train-dmem-look-pads-{tail}", "new_dropout_seed") == 6       # two attention seeds, four epilogue sites
        assert golden["cases"][f"mha-self-dropout-{tail}"]["bits"]["out0"] != golden["cases"][f"mha-self-{tail}"]["bits"]["out0"]
    a, b = golden["cases"]["mha-self-d512h1-f32"]["bits"], golden["cases"]["mha-self-d512h1-bf16"]["bits"]
    assert a["out0"] != b["out0"] and a["out1"] != b["out1"]


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--write":
        sys.exit("usage: python tests/test_attention_sublayer_bits_gpu.py --write <path>")
    _write(sys.argv[2])
