#!/usr/bin/env python3
"""bench.py — encoder frames/s of the LibriSpeech Conformer-SummaryMixing training step on MI355X.

    python bench.py --gpus 1 --steps 10 --warmup 3                      # default: config C2b, bf16 training step
    python bench.py --gpus 1 --steps 10 --warmup 3 --full               # + roofline, CPU baseline, extra points
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

A "step" = one pass of the hot path over one synthetic padded utterance batch per GPU: encoder forward
(input Linear + abs-sine PE + 12 Conformer-SummaryMixing layers + final LN), backward, gradient all-reduce
(N > 1), global-norm clip and fused AdamW — all in the hand-written gfx950 kernels of libsmx.so.  Inputs are
resident in HBM before the timed region.  Weak scaling: every rank processes its own (B, T) batch, the only
collective is the bucketed gradient all-reduce (RCCL over xGMI).

`python bench.py --gpus N` without a torchrun environment re-launches itself under torch.distributed.run with N ranks
(and fails loudly when fewer than N GPUs are visible).  --scaling strong keeps the GLOBAL batch fixed (B / N per rank).
--grad-accum G: one step = one OPTIMIZER step over G micro-batches (the recipe: 4 x 150 s), --accum sequential (G forward +
backward passes accumulate, the reference's fit_batch) or fused (trainer.fuse_microbatches: ONE batch, same gradients).
--dump-outputs DIR: after the timed steps, what the last one computed (encoder output; training: also the updated weights and
the gradients) as DIR/<name>.npy - the inputs are seeded, so two builds of the project compare output for output.

Prints ONE JSON line (rank 0) with the driver contract fields.  A plain run does only what they need: set up, warm up, time the
steps, --dump-outputs, print.  --full adds the measurements that take runs of their own (each can be left out again with
--no-roofline / --no-cpu-baseline / --no-extra-points):
  "roofline":     roofline of the DOMINANT KERNEL of the step: the kernel symbol (template instantiation, as rocprofv3 --stats
                  names it; GEMMs: asked of the library, smx_gemm_plan_query) with the largest share of the in-step kernel time,
                  averaged over all its launches inside one instrumented step: algorithmic bytes / HIP-event time on the stream
                  each launch ran on; its shapes, `traffic` (committed PMC passes, call-weighted) and the co-dominant symbols
                  ride along.  At d_model <= 512 every GEMM of this model sits below the bf16 ridge (~312 flop/B), so the bound
                  reported is HBM; the MFMA fraction is given alongside,
  "roofline_symbols": the same figures for the top symbols; "roofline_family": the gemm_kernel template as a whole,
  "roofline_step": the whole step: sum of the algorithmic bytes / flops of EVERY launch over the timed ms_per_step,
  "roofline_kernels": the top launches by shape + epilogue of that instrumented step: calls/step, in-step avg us,
                  algorithmic bytes per launch, fraction of the HBM roof, share of the step's kernel time,
  "roofline_isolated": the FFN up-projection GEMM and the dominant wgrad shape timed back to back in isolation,
  "roofline_pool": HBM roofline of the masked-mean pool kernel at the long-utterance point (config 5),
  "cpu_baseline": the oracle (PyTorch-CPU restatement of the reference graph) timed on this node's host cores
                  on a bounded sample of the same workload,
  "extra_points": (the default line only) the other batches SURVEY 8(d) defines and the bf16 residual stream, each a short
                  child run of this script.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

CONFIGS = {
    # BASELINE.json configs[1]: 12 layers, d_model 256 (SURVEY §8d "C2b").  Batch: 128 utterances x 500 encoder frames
    # (20 s each): the recipe sizes 150 s of audio per batch for a 24 GB card (...transducer.yaml:112-116), the same
    # rule gives ~1800-2600 s on 288 GB.  --batch 64 reproduces SURVEY's "saturating batch".
    "c2b": dict(kind="conformer", d=256, f=1024, l=256, layers=12, nhead=4, input=640, B=128, T=500,
                name="LibriSpeech Conformer-SummaryMixing C2b (12L, d_model=256, d_ffn=1024, SummaryMixing-fast, Swish)"),
    # recipe-faithful shapes of conformer_summarymixing_transducer.yaml:130-146 (SURVEY §8d "C2a")
    "c2a": dict(kind="conformer", d=512, f=2048, l=512, layers=12, nhead=4, input=640, B=128, T=500,
                name="LibriSpeech Conformer-SummaryMixing C2a (12L, d_model=512, d_ffn=2048, SummaryMixing-fast, Swish)"),
    # plumbing config 1
    "c1": dict(kind="conformer", d=144, f=576, l=144, layers=2, nhead=4, input=640, B=2, T=50,
               name="config-1 plumbing (2L, d_model=144)"),
    # Branchformer CommonVoice (config 4)
    "c4": dict(kind="branchformer", d=512, f=0, l=512, layers=18, nhead=1, input=640, B=128, T=250, csgu=3072,
               name="Branchformer-SummaryMixing CV (18L, d_model=512, csgu 3072)"),
    # BASELINE.json configs[4] / SURVEY §8d "C5": long-utterance stress, x (8, 30000, 512) N(0,1) straight into the
    # 12-layer encoder stack (no input Linear / PE: the reference's PE table ends at 2500 frames), forward only, ragged
    # lengths U(0.5,1).  With --seq-parallel under torchrun the TIME axis is sharded over the ranks (strong scaling).
    "c5": dict(kind="conformer", stack_only=True, d=512, f=2048, l=512, layers=12, nhead=4, input=512, B=8, T=30000,
               name="Long-utterance stress C5 (12L Conformer-SummaryMixing stack, d_model=512, d_ffn=2048, fast)"),
}
FLOPS_PER_FRAME_FWD = {"c2b": 36.7e6, "c2a": 145.7e6, "c5": 145.0e6}   # SURVEY §8(a) A12 (c5: without the input Linear)


def build_encoder(cfg, device, dropout=0.0):
    from summarymixing_amd.lobes.models.transformer.TransformerASR import EncoderWrapper, TransformerASR
    torch.manual_seed(3407)   # recipe seed (…transducer.yaml:12)
    kw = dict(tgt_vocab=1000, input_size=cfg["input"], d_model=cfg["d"], nhead=cfg["nhead"],
              num_encoder_layers=cfg["layers"], num_decoder_layers=0, dropout=dropout, attention_type="SummaryMixing",
              local_proj_hid_dim=[cfg["l"]], local_proj_out_dim=cfg["l"], summary_hid_dim=[cfg["l"]], causal=False,
              kernel_size=31)
    if cfg["kind"] == "conformer":
        net = TransformerASR(encoder_module="conformer", d_ffn=cfg["f"], mode="SummaryMixing-fast", **kw)
    else:
        net = TransformerASR(encoder_module="branchformer", mode="SummaryMixing", summary_out_dim=cfg["d"],
                             csgu_linear_units=cfg["csgu"], **kw)
    return EncoderWrapper(net).to(device).train()


def build_stack(cfg, device):
    """Config 5: the bare ConformerEncoder stack (eval)."""
    from summarymixing_amd.lobes.models.transformer.Conformer import ConformerEncoder
    torch.manual_seed(3407)
    enc = ConformerEncoder(cfg["layers"], cfg["d"], cfg["f"], cfg["nhead"], kernel_size=31, activation="swish", dropout=0.0,
                           attention_type="SummaryMixing", local_proj_hid_dim=[cfg["l"]], local_proj_out_dim=cfg["l"],
                           summary_hid_dim=[cfg["l"]], mode="SummaryMixing-fast")
    with torch.no_grad():
        for p in enc.parameters():
            if p.dim() > 1:
                torch.nn.init.xavier_normal_(p)
    return enc.to(device).eval()


def synthetic_batch(cfg, rank, device, dtype):
    g = torch.Generator().manual_seed(1234 + rank)
    B, T = cfg["B"], cfg["T"]
    src = torch.randn(B, T, cfg["input"], generator=g)
    wav_len = 0.5 + 0.5 * torch.rand(B, generator=g)
    wav_len[0] = 1.0
    valid = torch.arange(T)[None, :] < torch.round(wav_len * T)[:, None]
    src = src * valid[..., None]                     # zero padded frames, as real batches
    r = torch.randn(B, T, cfg["d"], generator=g) / (B * T)
    return src.to(device).to(dtype), wav_len.to(device), r.to(device).to(dtype), int(valid.sum())


def time_kernel(fn, iters=30, warm=5):
    """Average duration (s) of one launch, HIP events on the launch stream (torch's current stream)."""
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / iters


PMC_FILES = ("r06_pmc_traffic.txt", "r05_pmc_panel.txt", "r05_pmc_traffic.txt", "r05_pmc_wgrad_group.txt", "r04_pmc_traffic.txt", "r04_pmc_wgrad_group.txt", "r03_pmc_traffic.txt", "r03_pmc_wgrad_group.txt", "r02_pmc_traffic.txt", "r02_pmc_wgrad_group.txt", "r01_pmc_traffic.txt")
PMC_NOTE = ("HBM bytes per launch read from the COMMITTED PMC passes under profiles/ (TCC FETCH_SIZE x2-corrected + "
            "WRITE_SIZE, separate --pmc passes of tools/pmc_traffic.sh / pmc_panel.sh / pmc_wgroup.sh on this exact shape) - a constant of the build, "
            "not measured in this run; null when no pass exists for the shape")


def pmc_traffic_bytes(tag):
    """HBM bytes per launch from the committed PMC passes (profiles/r0N_pmc_traffic.txt), or None when no matching line."""
    import re
    lines = []
    for fn in PMC_FILES:
        try:
            lines += open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", fn)).readlines()
        except OSError:
            pass
    try:
        for line in lines:
            if tag in line:
                m = re.search(r"traffic\(corrected\)=([0-9.]+) MB", line)
                if m:
                    return float(m.group(1)) * 1e6
    except OSError:
        pass
    return None


def roofline_step_kernels(step, dtype, ms_per_step, top=8):
    """One instrumented (eager) step: every libsmx launch bracketed by HIP events on its own stream (ops._PROF).
    -> (roofline of the DOMINANT KERNEL SYMBOL - the instantiation a profiler lists first by share of the step's kernel time -,
        top launches by shape, per-symbol table, roofline of the gemm_kernel template as a whole, whole-step roofline)."""
    from summarymixing_amd import ops
    step()                                   # settle allocations of the eager path
    torch.cuda.synchronize()
    ops.prof_start()
    step()
    recs = ops.prof_stop(symbols=True)
    es = 2 if dtype == torch.bfloat16 else 4
    mfma_peak = 2500.0 if es == 2 else 157.3
    total_ms = sum(r[3] for r in recs) or 1e-9
    by_name, by_sym = {}, {}
    for name, nb, fl, ms, sym in recs:
        for d, k in ((by_name, name), (by_sym, sym)):
            e = d.setdefault(k, [0, 0.0, 0.0, 0.0])
            e[0] += 1; e[1] += nb; e[2] += fl; e[3] += ms

    def entry(k, e):
        calls, nb, fl, ms = e
        t = ms * 1e-3
        return {"kernel": k, "calls_per_step": calls, "in_step_avg_us": ms * 1e3 / calls, "algorithmic_bytes_per_launch": nb / calls,
                "hbm_GBps_algorithmic": nb / t / 1e9, "frac_hbm": nb / t / 1e9 / 8000.0, "mfma_TFLOPs": fl / t / 1e12,
                "frac_mfma": fl / t / 1e12 / mfma_peak, "share_of_step_kernel_time": ms / total_ms}
    kernels = [entry(k, e) for k, e in sorted(by_name.items(), key=lambda kv: -kv[1][3])[:top]]
    for k in kernels:                                  # HBM bytes from the committed PMC passes: the launch's full name first
        full = k["kernel"].strip()                     # (shape + epilogue, the round-3 passes), then the bare shape (rounds 1-2)
        tag = full.split(" +")[0].split(":")[0].strip()
        k["traffic"] = (pmc_traffic_bytes(full + " [") or
                        pmc_traffic_bytes("wgrad_group bf16 (8 weights" if tag.startswith("wgrad_group bf16 (8 weights") else tag))
    symbols = [entry(k, e) for k, e in sorted(by_sym.items(), key=lambda kv: -kv[1][3])[:top]]

    def roof_of(label, e, d):
        intensity = e[2] / max(e[1], 1.0)
        bound = "hbm" if intensity < mfma_peak * 1e12 / 8000e9 else "mfma"
        return {"kernel": label, "bound": bound, "unit": "GB/s" if bound == "hbm" else "TFLOP/s",
                "achieved": d["hbm_GBps_algorithmic"] if bound == "hbm" else d["mfma_TFLOPs"],
                "peak": 8000.0 if bound == "hbm" else mfma_peak,
                "frac": d["frac_hbm"] if bound == "hbm" else d["frac_mfma"],
                "launch_us": d["in_step_avg_us"], "calls_per_step": e[0], "share_of_step_kernel_time": d["share_of_step_kernel_time"],
                "algorithmic_bytes_per_launch": d["algorithmic_bytes_per_launch"], "arithmetic_intensity_flop_per_byte": intensity,
                "mfma_TFLOPs": d["mfma_TFLOPs"], "mfma_frac": d["frac_mfma"], "step_kernel_time_ms": total_ms}
    # headline: the kernel SYMBOL (the template instantiation rocprofv3 --stats lists first) with the largest share of the step's
    # kernel time, averaged over all its launches (its shapes differ: algorithmic bytes and duration are launch averages)
    top_sym, top_e = max(by_sym.items(), key=lambda kv: kv[1][3])
    roof = roof_of(top_sym + " (in-step average over its launches, HIP events on the launch stream)", top_e, symbols[0])
    shapes = sorted(((n, e) for n, e in by_name.items() if any(r[0] == n and r[4] == top_sym for r in recs)), key=lambda kv: -kv[1][3])
    roof["shapes"] = [{"launch": n.strip(), "calls_per_step": e[0], "in_step_avg_us": e[3] * 1e3 / e[0], "algorithmic_bytes_per_launch": e[1] / e[0],
                       "traffic": pmc_traffic_bytes(n.strip() + " [")} for n, e in shapes]
    tr = [(sh["traffic"], sh["calls_per_step"]) for sh in roof["shapes"]]
    roof["traffic"] = (sum(t * c for t, c in tr) / sum(c for _, c in tr)) if tr and all(t for t, _ in tr) else None
    roof["traffic_note"] = PMC_NOTE + "; call-weighted mean over the symbol's shapes"
    # symbols whose share is within 10 % (relative) of the headline's are listed next to it (which of two close ones leads changes
    # from box to box), and every other symbol of the top of the table follows in `roofline_symbols`
    top_share = symbols[0]["share_of_step_kernel_time"]
    roof["co_dominant"] = [dict(k) for k in symbols[1:] if k["share_of_step_kernel_time"] >= 0.9 * top_share]
    # the gemm_kernel TEMPLATE as a whole (every instantiation, every shape): the family view of rounds 1-4
    fe = [0, 0.0, 0.0, 0.0]
    for k, e in by_sym.items():
        if k.startswith("gemm_kernel<"):
            for i in range(4):
                fe[i] += e[i]
    fam_roof = roof_of(f"gemm_kernel<...> template (all {fe[0]} in-step launches of its instantiations)", fe, entry("gemm_kernel", fe)) if fe[0] else None
    # the whole step: every launch's algorithmic bytes and flops over the TIMED step (not the instrumented one)
    tb, tf = sum(r[1] for r in recs), sum(r[2] for r in recs)
    step_roof = {"ms_per_step": ms_per_step, "launches": len(recs), "algorithmic_bytes": tb, "flops": tf,
                 "hbm_GBps_algorithmic": tb / (ms_per_step * 1e-3) / 1e9, "frac_hbm": tb / (ms_per_step * 1e-3) / 1e9 / 8000.0,
                 "mfma_TFLOPs": tf / (ms_per_step * 1e-3) / 1e12, "frac_mfma": tf / (ms_per_step * 1e-3) / 1e12 / mfma_peak,
                 "note": "sum over every libsmx launch of one step (ops.gemm / row-kernel byte models, SURVEY 8(d)) / the timed ms_per_step; "
                         "peaks 8000 GB/s and the dense MFMA peak of the dtype"}
    return roof, kernels, symbols, fam_roof, step_roof


def roofline_wgrad(cfg, dtype):
    """The dominant wgrad shape (FFN weights, M x K = d_ffn x d) in isolation: slabs + fixed-order reduction."""
    from summarymixing_amd import ops
    N, K, M = cfg["B"] * cfg["T"], cfg["d"], cfg["f"] or 4 * cfg["d"]
    dz = torch.randn(N, M, device="cuda").to(dtype)
    x = torch.randn(N, K, device="cuda").to(dtype)
    gw = torch.zeros(M, K, device="cuda")
    gb = torch.zeros(M, device="cuda")
    t = time_kernel(lambda: ops.wgrad(dz, x, gw, N, M, K, dbias=gb))
    es = 2 if dtype == torch.bfloat16 else 4
    nb, fl = (M + K) * N * es + 4 * M * K, 2.0 * N * M * K
    return {"kernel": f"wgrad slabs + reduction dW({M}x{K}) over {N} frames (isolated, back to back)", "bound": "hbm",
            "launch_us": t * 1e6, "achieved": nb / t / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": nb / t / 1e9 / 8000.0,
            "algorithmic_bytes_per_launch": nb, "mfma_TFLOPs": fl / t / 1e12,
            "traffic": pmc_traffic_bytes(f"wgrad bf16 dW({M}x{K}) over {N}") if es == 2 else None, "traffic_note": PMC_NOTE}


def roofline_gemm(cfg, dtype):
    """The FFN up-projection GEMM (+bias+Swish+Z) in isolation, back to back: the panel-resident kernel where the product uses it
    (bf16, K = 256 / 512), else gemm_kernel<NT, 128x128>."""
    from summarymixing_amd import _lib as L, ops
    N, K, M = cfg["B"] * cfg["T"], cfg["d"], cfg["f"] or 4 * cfg["d"]
    x = torch.randn(N, K, device="cuda").to(dtype)
    w = (torch.randn(M, K, device="cuda") * 0.05).to(dtype)
    b = torch.randn(M, device="cuda")
    y, z = torch.empty(N, M, device="cuda", dtype=dtype), torch.empty(N, M, device="cuda", dtype=dtype)
    panel = dtype == torch.bfloat16 and ops.gemm_panel_ok(x, M, K)       # what the product launches for this Linear (functional.linear_fwd)
    if panel:
        wp, e = ops.weight_pack(w, bias=b), ops.epilogue(act=L.ACT_SWISH, z=z)
        t = time_kernel(lambda: ops.gemm_panel(x, wp, y, N, M, K, e))
    else:
        e = ops.epilogue(bias=b, act=L.ACT_SWISH, z=z)
        t = time_kernel(lambda: ops.gemm(L.GEMM_NT, x, w, y, N, M, K, e))
    flops = 2.0 * N * K * M
    es = 2 if dtype == torch.bfloat16 else 4
    mfma_peak = 2500.0 if dtype == torch.bfloat16 else 157.3
    alg_bytes = (N * K + M * K + 2 * N * M) * es + 4 * M      # X + W + Y + Z + bias (SURVEY §8d per-unit figures)
    intensity = flops / alg_bytes                              # flop per algorithmic byte
    ridge = mfma_peak * 1e12 / 8000e9                          # ~312 flop/B (bf16): below it the kernel is HBM-bound
    name = ((f"gemm_panel_kernel<{K}, 0, {L.ACT_SWISH}>" if panel else f"gemm_kernel<{'bf16' if es == 2 else 'f32'},NT,128x128>") +
            f" FFN up-proj ({N}x{K})x({K}x{M}) +bias+swish+Z")
    common = {"kernel": name, "launch_us": t * 1e6, "arithmetic_intensity_flop_per_byte": intensity,
              "mfma_TFLOPs": flops / t / 1e12, "mfma_frac": flops / t / 1e12 / mfma_peak,
              "hbm_GBps_algorithmic": alg_bytes / t / 1e9,
              "traffic": pmc_traffic_bytes(f"gemm NT bf16 ({N}x{K})x({K}x{M})") if es == 2 else None,
              "traffic_note": PMC_NOTE + f"; algorithmic bytes {alg_bytes / 1e6:.1f} MB"}
    if intensity < ridge:
        return dict(common, bound="hbm", achieved=alg_bytes / t / 1e9, peak=8000.0, unit="GB/s",
                    frac=alg_bytes / t / 1e9 / 8000.0)
    return dict(common, bound="mfma", achieved=flops / t / 1e12, peak=mfma_peak, unit="TFLOP/s",
                frac=flops / t / 1e12 / mfma_peak)


def roofline_pool(dtype):
    """Config 5 roofline point: masked mean over (B=8, T=30000, D=512); algorithmic bytes per launch =
    B*T*D*sizeof + B*T (mask) + 4*B*D."""
    from summarymixing_amd import ops
    B, T, D = 8, 30000, 512
    s = torch.randn(B * T, D, device="cuda").to(dtype)
    lens = torch.randint(T // 2, T + 1, (B,), device="cuda")
    lens[0] = T
    mask = (torch.arange(T, device="cuda")[None] < lens[:, None]).reshape(-1).view(torch.uint8)
    t = time_kernel(lambda: ops.masked_mean(s, mask, B, T, True, False))
    es = 2 if dtype == torch.bfloat16 else 4
    nbytes = B * T * D * es + B * T + 4 * B * D
    return {"kernel": f"masked_sum_stage1+2 ({B},{T},{D}) {'bf16' if es == 2 else 'f32'}", "bound": "hbm",
            "achieved": nbytes / t / 1e9, "peak": 8000.0, "unit": "GB/s", "frac": nbytes / t / 1e9 / 8000.0,
            "traffic": pmc_traffic_bytes(f"pool {'bf16' if es == 2 else 'f32 '} ({B},{T},{D})"), "launch_us": t * 1e6}


def cpu_model():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def cpu_baseline(cfg, train):
    """The oracle (PyTorch-CPU restatement of the reference module graph) on a bounded sample of the same
    workload: same model shapes, fp32, B=4 utterances of the same T (about 10-30 s of CPU work).  Timed at
    min(all cores, 32) threads (the reported value) and at 8 threads."""
    from oracle import smx_oracle as O
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or (os.cpu_count() or 1)
    except Exception:                                     # noqa: BLE001
        phys = max(1, (os.cpu_count() or 2) // 2)
    # "all physical cores and n = 8"; torch CPU scales poorly past ~32 threads on these small GEMMs, so 32 is
    # timed as well and the BEST of the three is the reported value (the 32-thread value flattered the GPU)
    thread_counts = sorted({min(8, phys), min(32, phys), phys})
    cores = thread_counts[0]
    torch.set_num_threads(cores)
    if cfg.get("stack_only"):
        return cpu_baseline_stack(cfg, min(32, phys))
    enc = build_encoder(cfg, "cpu")
    sd = {k: v.detach().clone().requires_grad_(train and v.is_floating_point())
          for k, v in enc.transformer.state_dict().items() if k != "positional_encoding.pe"}
    small = dict(cfg, B=min(cfg["B"], 4))
    src, wav_len, r, _ = synthetic_batch(small, 0, "cpu", torch.float32)
    kind = "conformer" if cfg["kind"] == "conformer" else "branchformer"
    act = "swish" if kind == "conformer" else "gelu"
    mode = "SummaryMixing-fast" if kind == "conformer" else "SummaryMixing"

    def step():
        y = O.asr_encode(src, wav_len, sd, kind, act, mode, cfg["l"])
        if train:
            y.backward(r)
            for v in sd.values():
                v.grad = None
    def timed(budget):
        t0 = time.perf_counter()
        step()                                   # warm-up, also bounds the sample
        first = time.perf_counter() - t0
        t0 = time.perf_counter()
        n = 0
        while n < 1 or (n < 20 and time.perf_counter() - t0 + first < budget):
            step()
            n += 1
        return (time.perf_counter() - t0) / n, n
    frames = small["B"] * small["T"]
    by_threads = {}
    for nt in thread_counts:
        torch.set_num_threads(nt)
        dt, n = timed(8.0 if nt == thread_counts[0] else 6.0)
        by_threads[nt] = (frames / dt, n)
    best = max(by_threads, key=lambda k: by_threads[k][0])
    return {"value": by_threads[best][0], "unit": "encoder frames/s", "cores": best, "kind": "port", "cpu_model": cpu_model(),
            "host_cpus": os.cpu_count(), "physical_cores": phys,
            "frames_per_s_by_threads": {str(k): v[0] for k, v in by_threads.items()},
            "sample": f"oracle/smx_oracle.py asr_encode {'fwd+bwd' if train else 'fwd'}, fp32, B={small['B']} x T={small['T']} "
                      f"of the same model, {by_threads[best][1]} steps, torch {torch.__version__}; best of "
                      f"{thread_counts} threads = {best}"}


def cpu_baseline_stack(cfg, cores):
    """Config 5 on the host: the oracle's ConformerEncoder forward on ONE utterance of 3000 frames of the same model."""
    from oracle import smx_oracle as O
    enc = build_stack(cfg, "cpu")
    sd = {k: v.detach() for k, v in enc.state_dict().items()}
    T = 3000
    x = torch.randn(1, T, cfg["d"], generator=torch.Generator().manual_seed(1234))
    pad = torch.ones(1, T, dtype=torch.bool)

    def step():
        with torch.no_grad():
            O.conformer_encoder(x, sd, "", "swish", "SummaryMixing-fast", cfg["l"], None, pad)
    step()
    t0 = time.perf_counter()
    n = 0
    while n < 1 or (n < 20 and time.perf_counter() - t0 < 12.0):
        step()
        n += 1
    dt = (time.perf_counter() - t0) / n
    return {"value": T / dt, "unit": "encoder frames/s", "cores": cores, "kind": "port",
            "sample": f"oracle/smx_oracle.py conformer_encoder fwd, fp32, 1 x {T} frames of the same stack, {n} passes, "
                      f"torch {torch.__version__}, {cores} threads"}


def gpu_topology():
    """One line per GPU pair class as rocm-smi reports it (link type / hops), once, for the record of a multi-GPU run."""
    try:
        r = subprocess.run(["rocm-smi", "--showtopotype"], capture_output=True, text=True, timeout=20)
        lines = [ln.strip() for ln in r.stdout.splitlines() if ln.strip() and not ln.startswith("=")]
        return lines[:12]
    except Exception as ex:                                # noqa: BLE001 - the topology is a note, never a failure
        return [f"rocm-smi unavailable: {type(ex).__name__}"]


def rccl_env():
    """The RCCL / NCCL / HSA variables this process sees (what shaped the collectives of a multi-GPU run)."""
    keys = sorted(k for k in os.environ if k.startswith(("NCCL_", "RCCL_", "HSA_", "HIP_VISIBLE", "ROCR_VISIBLE")))
    return {k: os.environ[k] for k in keys}


def want_graph_for(args, cfg, train, dist_run):
    """The launch mode bench.py would pick (mirrors main()): (hipGraph?, reason)."""
    want = args.graph == "on" or (args.graph == "auto" and cfg["B"] * cfg["T"] < 40000)
    if not want:
        return False, "eager: >= 40000 frames per GPU hide the host launch path behind the kernels"
    if train and dist_run and args.reduce == "rs_ag":
        return False, "eager: the sharded update (reduce-scatter / all-gather inside the step) stays out of graphs"
    if train and dist_run:
        return True, "two graphs [zero_grad + forward + backward] | ONE eager RCCL all-reduce of the flat gradients | [clip + AdamW]"
    return True, "one graph of the whole step"


def dp_plan(args, world):
    """The data-parallel plan of `--gpus world` WITHOUT GPUs: model and flat layout on the CPU (same constructor, same
    parameter order), buckets / shards from summarymixing_amd.trainer.plan_buckets / shard_map."""
    from summarymixing_amd.trainer import ALIGN, FlatAdamW, plan_buckets, shard_map
    cfg = dict(CONFIGS[args.config])
    if args.batch:
        cfg["B"] = args.batch
    if args.frames:
        cfg["T"] = args.frames
    if cfg.get("stack_only"):
        raise SystemExit("--dry-run-ranks: config c5 is forward-only (no gradient exchange)")
    enc = build_encoder(cfg, torch.device("cpu"), 0.0)
    opt = FlatAdamW(enc, compute_dtype=torch.float32)      # (CPU: flat layout only, no kernels)
    layer_ranges = [opt.param_range(list(l.parameters())) for l in enc.transformer.encoder.layers]
    buckets = plan_buckets(opt.total, layer_ranges)
    gsz = 2 if args.grad_dtype == "bf16" else 4
    shards = shard_map(buckets, world)
    covered = sum(b - a for a, b, _ in buckets)
    graph, why = want_graph_for(args, cfg, True, world > 1)
    gb = opt.total * gsz
    return {
        "dry_run_ranks": world, "config": args.config, "per_gpu_batch": cfg["B"], "enc_frames_per_utt": cfg["T"],
        "parameters": sum(p.numel() for p in opt.params), "flat_elements": opt.total, "align_elements": ALIGN,
        "reduce": args.reduce, "grad_dtype": args.grad_dtype,
        "buckets_in_launch_order": [{"name": n, "start": a, "end": b, "wire_dtype_bytes": (b - a) * gsz} for a, b, n in buckets],
        "buckets_cover_flat_buffer_exactly_once": covered == opt.total and len({(a, b) for a, b, _ in buckets}) == len(buckets),
        "rs_ag_shards_rank0": shards[0], "rs_ag_shard_elements_per_rank": [sum(b - a for a, b in shards[r]) for r in range(world)],
        "wire_bytes_per_rank_per_step": (2.0 * (world - 1) / world * gb if args.reduce == "allreduce"
                                         else (world - 1) / world * (gb + opt.total * 4)),
        "xgmi_ring_floor_ms_at_153GBps_per_link": (2.0 * (world - 1) / world * gb) / 153e9 * 1e3 if world > 1 else 0.0,
        "hipgraph": graph, "launch_mode": why, "rccl_env": rccl_env(),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", default="c2b", choices=sorted(CONFIGS))
    ap.add_argument("--mode", default="train", choices=["train", "forward"])
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--frames", type=int, default=None)
    ap.add_argument("--dropout", type=float, default=0.15, help="training-mode dropout (recipe: 0.15)")
    ap.add_argument("--graph", default="auto", choices=["auto", "on", "off"],
                    help="capture the step once in a hipGraph and replay it (auto: single-GPU runs below 40000 frames per step, "
                         "where the host launch path is the bottleneck; neutral above)")
    ap.add_argument("--seq-parallel", action="store_true",
                    help="config c5 under torchrun: shard the TIME axis over the ranks (summarymixing_amd/sequence_parallel.py) "
                         "instead of the utterances; the job then processes ONE batch (strong scaling)")
    ap.add_argument("--scaling", default="weak", choices=["weak", "strong"],
                    help="weak: every rank runs the config's batch (default); strong: the GLOBAL batch is the config's batch, "
                         "each of the N ranks gets B / N utterances")
    ap.add_argument("--dynchunk", default=None, metavar="CHUNK[,LEFT]",
                    help="Dynamic Chunk Training batch (…transducer.yaml:84-91): chunk size in encoder frames and, optionally, the "
                         "left context in chunks (default: unlimited) - chunked summary means and Dynamic Chunk Convolution")
    ap.add_argument("--reduce", default="allreduce", choices=["allreduce", "rs_ag"],
                    help="gradient exchange of the data-parallel step (trainer.FlatAdamW): one all-reduce per layer bucket, or "
                         "reduce-scatter + sharded AdamW + all-gather of the weights")
    ap.add_argument("--grad-dtype", default="fp32", choices=["fp32", "bf16"], help="dtype of the gradients on the wire (xGMI)")
    ap.add_argument("--grad-accum", type=int, default=1, metavar="G",
                    help="micro-batches per optimizer step (the recipe: grad_accumulation_factor 4 x max_batch_len 150 s)")
    ap.add_argument("--accum", default="sequential", choices=["sequential", "fused"],
                    help="sequential: G forward+backward passes accumulate, one update (the reference's fit_batch); fused: the G "
                         "micro-batches run as ONE batch (trainer.fuse_microbatches: same gradients, sized for 288 GB)")
    ap.add_argument("--full", action="store_true",
                    help="after the result line's own fields, also measure the roofline objects, the CPU baseline and (default line) "
                         "the extra_points; a plain run only sets up, warms up, times the steps and writes --dump-outputs")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip cpu_baseline")
    ap.add_argument("--no-extra-points", action="store_true",
                    help="(--full) skip the extra_points of the default line (SURVEY 8d batches: C2b B=64 x 500, C2a B=10 x 375, and "
                         "the bf16 residual stream), each a short child run of this script")
    ap.add_argument("--no-roofline", action="store_true", help="(--full) skip the roofline objects")
    ap.add_argument("--roofline-step-only", action="store_true",
                    help="(--full; the extra_points child runs) only roofline_step - the step's algorithmic bytes / flops over the timed "
                         "step - instead of the per-kernel roofline objects")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write what the last one computed as DIR/<name>.npy (float32; rank 0): the encoder "
                         "output and, when training, the updated weights and the gradients - at most 60 MiB in all, larger arrays as a "
                         "fixed sample of their elements (dump_outputs)")
    ap.add_argument("--dry-run-ranks", type=int, default=0, metavar="N",
                    help="no GPU needed: build the model on the CPU, print the N-rank data-parallel plan (gradient buckets in "
                         "launch order, the rs_ag shard map, bytes on the wire, the hipGraph split decision, the RCCL environment) "
                         "as one JSON line and exit")
    args = ap.parse_args()
    if args.dry_run_ranks:
        print(json.dumps(dp_plan(args, args.dry_run_ranks)))
        return

    if args.gpus > 1 and "RANK" not in os.environ:
        # plain `python bench.py --gpus N`: become N ranks (one process per GPU) under torch.distributed.run
        import socket
        import subprocess
        ndev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if ndev < args.gpus:
            raise SystemExit(f"bench.py --gpus {args.gpus}: only {ndev} GPU(s) visible on this node - refusing to run fewer ranks "
                             "than asked for")
        sk = socket.socket()
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
        sk.close()
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
               "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd).returncode)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X: the product path has no CPU fallback")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    force_dist = os.environ.get("SMX_FORCE_ALLREDUCE") == "1" and "RANK" in os.environ
    if world > 1 or force_dist:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("NCCL_DEBUG", "VERSION")     # RCCL prints its version line once (stderr) - kept with the run's log
        dist.init_process_group("nccl", device_id=dev)
    if world != args.gpus:
        raise SystemExit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks")
    if world > 1 or force_dist:
        world = torch.distributed.get_world_size()          # n_gpus = the ranks that really joined the RCCL group

    cfg = dict(CONFIGS[args.config])
    if args.batch:
        cfg["B"] = args.batch
    if args.frames:
        cfg["T"] = args.frames
    global_B = cfg["B"] * world
    if args.scaling == "strong":
        if cfg["B"] % world:
            raise SystemExit(f"--scaling strong: the global batch {cfg['B']} does not divide over {world} ranks")
        global_B = cfg["B"]
        cfg["B"] //= world
    dtype = torch.bfloat16 if args.dtype == "bf16" else torch.float32
    train = args.mode == "train"
    if cfg.get("stack_only"):
        return main_stack(args, cfg, dtype, dev, rank, world)
    if args.seq_parallel:
        raise SystemExit("--seq-parallel is the long-utterance mode of --config c5")

    from summarymixing_amd.trainer import FlatAdamW
    enc = build_encoder(cfg, dev, args.dropout if train else 0.0)
    opt = None
    if train:
        opt = FlatAdamW(enc, lr=8e-4, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01, max_grad_norm=5.0,
                        compute_dtype=dtype, reduce=args.reduce,
                        grad_dtype=torch.bfloat16 if args.grad_dtype == "bf16" else torch.float32)
        if world > 1 or force_dist:   # one gradient bucket per encoder layer, reduced as soon as its backward is done
            for layer in enc.transformer.encoder.layers:
                rng = opt.param_range(list(layer.parameters()))
                layer._on_bwd_done = (lambda r=rng: opt.reduce_bucket_async(*r))
    else:
        enc.eval()
    G = max(1, args.grad_accum)
    micro = [synthetic_batch(cfg, rank * G + g, dev, dtype) for g in range(G)]
    valid_frames = sum(m[3] for m in micro)
    if G > 1 and args.accum == "fused":
        from summarymixing_amd.trainer import fuse_microbatches
        src_f, wl_f = fuse_microbatches([(m[0], m[1]) for m in micro])
        micro = [(src_f, wl_f, torch.cat([m[2] for m in micro]), valid_frames)]
    src, wav_len, r = micro[0][:3]
    enc_kw = {}
    if args.dynchunk:
        from summarymixing_amd.utils.dynamic_chunk_training import DynChunkTrainConfig
        parts = [int(x) for x in args.dynchunk.split(",")]
        enc_kw["dynchunktrain_config"] = DynChunkTrainConfig(parts[0], parts[1] if len(parts) > 1 else None)

    latest = {}    # the encoder output of the latest step (--dump-outputs; under a hipGraph: the tensor every replay rewrites)

    def fwd_bwd_all():
        # (gradient accumulation: the kernels ADD into the flat gradient buffer; the bucket hooks fire on the last micro-batch only)
        opt.zero_grad()
        with opt.no_sync():
            for s_, wl_, r_, _ in micro[:-1]:
                enc(s_, wl_, **enc_kw).backward(r_)
        s_, wl_, r_, _ = micro[-1]
        y = enc(s_, wl_, **enc_kw)
        y.backward(r_)
        latest["encoder_out"] = y.detach()

    def step():
        if train:
            fwd_bwd_all()
            if world > 1 or force_dist:   # parameters outside the layer buckets (input Linear, final LN)
                first = opt.param_range(list(enc.transformer.encoder.layers[0].parameters()))[0]
                last = opt.param_range(list(enc.transformer.encoder.layers[-1].parameters()))[1]
                if first > 0:
                    opt.reduce_bucket_async(0, first)
                if last < opt.total:
                    opt.reduce_bucket_async(last, opt.total)
            opt.step()
        else:
            with torch.no_grad():
                latest["encoder_out"] = enc(src, wav_len, **enc_kw)

    def barrier():
        if world > 1 or force_dist:
            torch.distributed.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    barrier()
    # hipGraph: the ~1100 kernel launches of a step cost ~14 ms of host time - hidden behind the GPU at 64000 frames per
    # step, the bottleneck below ~30000.  One capture (after the eager warm-up has created gradients, shadows and
    # workspaces), then every timed step is one graph launch.  The step count (AdamW bias correction) and the dropout
    # epoch live in a device counter, so replays still advance them (include/smx.h: smx_step_counter_add).
    run, graph_note = step, "eager"
    dist_run = world > 1 or force_dist
    want_graph = args.graph == "on" or (args.graph == "auto" and micro[0][0].shape[0] * cfg["T"] < 40000)
    if want_graph and train and dist_run and args.reduce == "rs_ag":
        want_graph = False                                # (the sharded update holds collectives: kept out of graphs)
    if want_graph and train and dist_run:
        # data parallel: two graphs with the collective between them - [zero_grad + forward + backward] | ONE all-reduce of
        # the flat gradient buffer (eager, RCCL) | [clip + AdamW + shadow refresh].  The per-layer bucket hooks (overlap of
        # the all-reduce with the backward) are given up in this mode: it is for per-GPU batches so small that the host
        # launch path, not the GPU, bounds the step.
        try:
            opt.use_device_step_counter(True)
            for layer in enc.transformer.encoder.layers:
                layer._on_bwd_done = None

            fwd_bwd = fwd_bwd_all
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fwd_bwd()
                opt.all_reduce_all()
                opt.update_only()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g_a, g_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            # (thread_local: the RCCL watchdog thread polls the events of the warm-up collectives with hipEventQuery - in the default
            #  global capture mode that call from ANOTHER thread aborts the process while a capture is open)
            with torch.cuda.graph(g_a, capture_error_mode="thread_local"):
                fwd_bwd()
            with torch.cuda.graph(g_b, capture_error_mode="thread_local"):
                opt.update_only()

            def run():
                g_a.replay()
                opt.all_reduce_all()
                g_b.replay()
            graph_note = "hipGraph replay x2 (forward+backward | one RCCL all-reduce of the flat gradients | update)"
        except Exception as ex:                          # noqa: BLE001
            if args.graph == "on":
                raise
            opt.use_device_step_counter(False)
            torch.cuda.synchronize()
            run, graph_note = step, f"eager (hipGraph capture failed: {type(ex).__name__})"
    elif want_graph and not dist_run:
        try:
            if train:
                opt.use_device_step_counter(True)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()                                   # (untimed) allocate this stream's workspaces before capture
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            run, graph_note = graph.replay, "hipGraph replay (one capture of the whole step)"
        except Exception as ex:                          # noqa: BLE001 - report and time the eager path instead
            if args.graph == "on":
                raise
            if train:
                opt.use_device_step_counter(False)
            torch.cuda.synchronize()
            run, graph_note = step, f"eager (hipGraph capture failed: {type(ex).__name__})"
    if opt is not None and dist_run:
        opt.measure_comm(True)
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        run()
    barrier()
    dt = time.perf_counter() - t0
    if args.dump_outputs and rank == 0:          # (before the roofline's instrumented steps move the weights on)
        dump_outputs(args.dump_outputs, dict(latest, **({"parameters": opt.flat_p, "gradients": opt.flat_g} if train else {})))
    if world > 1 or force_dist:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    replica_check = None
    if (world > 1 or force_dist) and opt is not None:
        # data-parallel self-check, AFTER the timed region: every rank's parameters must be bit-identical (same init, the same
        # all-reduced gradients, the same update) - each rank contributes a checksum of its flat fp32 master buffer (sum and sum
        # of squares in float64 + the first / last elements), rank 0 compares
        fp = opt.flat_p.double()
        mine = torch.stack([fp.sum(), (fp * fp).sum(), fp[0], fp[-1], torch.tensor(float(opt.total), device=dev, dtype=torch.float64)])
        allc = [torch.zeros_like(mine) for _ in range(world)]
        torch.distributed.all_gather(allc, mine)
        same = all(torch.equal(c, allc[0]) for c in allc)
        replica_check = {"ranks": world, "identical_parameters": bool(same), "checksum_rank0": [float(v) for v in allc[0][:2]]}
        if rank == 0 and not same:
            raise SystemExit(f"bench.py: data-parallel replicas DIVERGED after {args.steps + args.warmup} steps: "
                             + "; ".join(f"rank {i}: {[float(v) for v in c]}" for i, c in enumerate(allc)))

    frames_per_step = cfg["B"] * cfg["T"] * world * G
    value = frames_per_step * args.steps / dt
    out = {
        "metric": "encoder frames/s (whole node), " + ("LibriSpeech Conformer-SummaryMixing" if cfg["kind"] == "conformer"
                                                       else "CommonVoice Branchformer-SummaryMixing"),
        "value": value, "unit": "encoder frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
        "dtype": args.dtype, "data": "synthetic",
        "config": {"workload": cfg["name"] + (" training step (fwd+bwd+grad-clip+AdamW)" if train else " forward"),
                   "per_gpu_batch": cfg["B"], "enc_frames_per_utt": cfg["T"], "global_batch": global_B,
                   "grad_accumulation": ({"micro_batches": G, "mode": args.accum,
                                          "utterances_per_launch": int(micro[0][0].shape[0])} if G > 1 else None),
                   "padded_frames_per_step": frames_per_step, "valid_frames_rank0": valid_frames,
                   "input": f"(B,T,{cfg['input']}) N(0,1), wav_len U(0.5,1), zero padded",
                   "dropout": (args.dropout if train else 0.0), "parallelism": f"dp{world}", "init": "xavier_normal seed 3407",
                   "residual_stream": ("float32 (torch autocast semantics, the reference's `precision: bf16`)" if F_stream_f32(dtype)
                                       else ("bf16 (SMX_RESIDUAL=bf16)" if dtype == torch.bfloat16 else "float32 model")),
                   "dynchunk": ({"chunk_size": enc_kw["dynchunktrain_config"].chunk_size,
                                 "left_context_chunks": enc_kw["dynchunktrain_config"].left_context_size} if enc_kw else None),
                   "launch": graph_note},
    }
    if args.config in FLOPS_PER_FRAME_FWD:
        fl = FLOPS_PER_FRAME_FWD[args.config] * (3.0 if train else 1.0)
        out["model_tflops"] = value * fl / 1e12
    if opt is not None:
        # data-parallel exchange: what crosses xGMI per step and how much of it the backward pass did NOT hide (time the
        # compute stream stood waiting for the collectives, mean over the timed steps, max over ranks)
        ce = opt.comm_exposed_ms() if dist_run else 0.0
        if world > 1 or force_dist:
            ct = torch.tensor([ce], device=dev, dtype=torch.float64)
            torch.distributed.all_reduce(ct, op=torch.distributed.ReduceOp.MAX)
            ce = float(ct.item())
        gb = opt.total * (2 if args.grad_dtype == "bf16" else 4)
        ce_ranks = [ce]
        if world > 1 or force_dist:                       # every rank's own figure (a straggler shows here, not in the max)
            ca = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(world)]
            torch.distributed.all_gather(ca, torch.tensor([opt.comm_exposed_ms() if dist_run else 0.0], device=dev, dtype=torch.float64))
            ce_ranks = [float(c.item()) for c in ca]
        from summarymixing_amd.trainer import plan_buckets
        gsz = 2 if args.grad_dtype == "bf16" else 4
        plan = plan_buckets(opt.total, [opt.param_range(list(l.parameters())) for l in enc.transformer.encoder.layers])
        out["comm"] = {"reduce": args.reduce, "grad_dtype": args.grad_dtype, "buckets": len(plan),
                       "bucket_bytes_in_launch_order": [(b - a) * gsz for a, b, _ in plan],
                       "comm_exposed_ms_per_rank": ce_ranks, "rccl_env": rccl_env(),
                       "gradient_bytes_per_rank": gb,
                       "wire_bytes_per_rank": (2.0 * (world - 1) / world * gb if args.reduce == "allreduce"
                                               else (world - 1) / world * (gb + opt.total * 4)),
                       "comm_exposed_ms": ce}
        out["comm_exposed_ms"] = ce
        if replica_check is not None:
            out["comm"]["replica_check"] = replica_check
            out["comm"]["rccl_version"] = ".".join(str(v) for v in torch.cuda.nccl.version()) if hasattr(torch.cuda, "nccl") else None
            out["comm"]["topology"] = gpu_topology()
    if rank == 0:
        if args.full:     # measurements of their own, after --dump-outputs (the instrumented steps move the weights on)
            if args.roofline_step_only and train and world == 1 and not force_dist:
                out["roofline_step"] = roofline_step_kernels(step, dtype, dt / args.steps * 1e3)[4]
            elif not args.no_roofline:
                if train and world == 1 and not force_dist:
                    (out["roofline"], out["roofline_kernels"], out["roofline_symbols"], out["roofline_family"],
                     out["roofline_step"]) = roofline_step_kernels(step, dtype, dt / args.steps * 1e3)
                    out["roofline_isolated"] = [roofline_wgrad(cfg, dtype), roofline_gemm(cfg, dtype)]
                else:
                    out["roofline"] = roofline_gemm(cfg, dtype)
                out["roofline_pool"] = roofline_pool(dtype)
            if not args.no_cpu_baseline and world == 1:
                out["cpu_baseline"] = cpu_baseline(cfg, train)
            default_line = (args.config == "c2b" and train and world == 1 and not force_dist and args.batch is None
                            and args.frames is None and args.dtype == "bf16" and not args.dynchunk)
            if default_line and not args.no_extra_points:
                out["extra_points"] = extra_points()
        print(json.dumps(out), flush=True)
    if world > 1 or force_dist:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


DUMP_BYTES = 60 << 20


def dump_outputs(path, arrays):
    """--dump-outputs: every array as <path>/<name>.npy in float32, DUMP_BYTES in all.  An array over its share keeps a fixed
    sample of its elements - flat indices drawn by a CPU generator of seed 0, sorted - the same from run to run and build to build,
    so two dumps of one command compare element for element."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    cap = DUMP_BYTES // 4 // len(arrays)
    for name, t in arrays.items():
        t = t.detach()
        if t.numel() > cap:
            idx = torch.randint(t.numel(), (cap,), generator=torch.Generator().manual_seed(0)).sort().values
            t = t.reshape(-1)[idx.to(t.device)]
        np.save(os.path.join(path, name + ".npy"), t.float().cpu().numpy())


def F_stream_f32(dtype):
    from summarymixing_amd import functional as F
    return dtype == torch.bfloat16 and F.stream_dtype(dtype) == torch.float32


def extra_points():
    """Short child runs of this script (free of this process's allocations): the batches SURVEY 8(d) defines next to the
    headline's B = 128 x 500, and the headline config on the bf16 residual stream."""
    import subprocess
    pts = []
    runs = (("C2b B=64 x T=500 (SURVEY 8d saturating batch)", ["--config", "c2b", "--batch", "64"], {}),
            ("C2a recipe batch B=10 x T=375 (150 s of audio, ...transducer.yaml:116)", ["--config", "c2a", "--batch", "10", "--frames", "375"], {}),
            ("C2a recipe OPTIMIZER step: 4 micro-batches of 10 x 375 (grad_accumulation_factor 4, ...transducer.yaml:65-66) as one fused "
             "batch (trainer.fuse_microbatches); ms_per_step is per optimizer step",
             ["--config", "c2a", "--batch", "10", "--frames", "375", "--grad-accum", "4", "--accum", "fused"], {}),
            ("C2b ONE utterance B=1 x T=500 (hipGraph replay of the whole step)", ["--config", "c2b", "--batch", "1", "--steps", "30"], {}),
            ("C2b B=128 x T=500 on the bf16 residual stream (SMX_RESIDUAL=bf16, rounds 1-2)", ["--config", "c2b"], {"SMX_RESIDUAL": "bf16"}))
    for label, extra, env in runs:
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", "10", "--warmup", "4", "--full", "--no-cpu-baseline",
               "--roofline-step-only", "--no-extra-points"] + extra
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=dict(os.environ, **env))
            d = json.loads(r.stdout.strip().splitlines()[-1])
            pts.append({"point": label, "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"],
                        "launch": d["config"]["launch"], "residual_stream": d["config"]["residual_stream"],
                        "roofline_step": d.get("roofline_step")})
        except Exception as ex:                          # noqa: BLE001
            pts.append({"point": label, "error": f"{type(ex).__name__}: {ex}"[:200]})
    return pts


def main_stack(args, cfg, dtype, dev, rank, world):
    """Config 5: encoder-stack forward on (B, T, d).  Default: every rank runs its own batch (weak scaling, no
    collective).  --seq-parallel: one batch, time axis sharded, two small exchanges per layer."""
    import contextlib
    from summarymixing_amd import sequence_parallel as SP
    enc = build_stack(cfg, dev)
    sp = args.seq_parallel and world > 1
    B, T = cfg["B"], cfg["T"]
    g = torch.Generator().manual_seed(1234 + (0 if sp else rank))
    x = torch.randn(B, T, cfg["d"], generator=g)
    lens = torch.round((0.5 + 0.5 * torch.rand(B, generator=g)) * T).long()
    lens[0] = T
    pad = torch.arange(T)[None, :] < lens[:, None]
    x = (x * pad[..., None]).to(dev).to(dtype)
    pad = pad.to(dev)
    ctx = SP.sequence_parallel() if sp else contextlib.nullcontext()
    with ctx:
        if sp:
            x, pad = SP.shard(x), SP.shard(pad)

        latest = {}

        def step():
            with torch.no_grad():
                latest["encoder_out"] = enc(x, src_key_padding_mask=pad)[0]

        def barrier():
            if world > 1:
                torch.distributed.barrier()
            torch.cuda.synchronize()
        for _ in range(args.warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        barrier()
        dt = time.perf_counter() - t0
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, latest)
    if world > 1:
        tt = torch.tensor([dt], device=dev, dtype=torch.float64)
        torch.distributed.all_reduce(tt, op=torch.distributed.ReduceOp.MAX)
        dt = float(tt.item())
    frames_per_step = B * T * (1 if sp else world)
    value = frames_per_step * args.steps / dt
    out = {"metric": "encoder frames/s (whole node), long-utterance Conformer-SummaryMixing encoder stack forward",
           "value": value, "unit": "encoder frames/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
           "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True, "scaling": "strong" if sp else "weak",
           "vs_baseline": None, "dtype": args.dtype, "data": "synthetic",
           "config": {"workload": cfg["name"] + " forward", "per_gpu_batch": B, "enc_frames_per_utt": T if not sp else T // world,
                      "padded_frames_per_step": frames_per_step, "valid_frames": int(lens.sum()),
                      "input": f"(B,T,{cfg['d']}) N(0,1) into the encoder stack, lengths U(0.5,1), zero padded",
                      "parallelism": (f"sp{world} (time axis sharded)" if sp else f"dp{world}"), "launch": "eager",
                      "residual_stream": ("float32 (torch autocast semantics)" if (F_stream_f32(dtype) and not sp) else
                                          ("bf16" if dtype == torch.bfloat16 else "float32 model"))},
           "model_tflops": value * FLOPS_PER_FRAME_FWD["c5"] / 1e12}
    if rank == 0:
        if args.full and not args.no_roofline:
            out["roofline"] = roofline_pool(dtype)
        if args.full and not args.no_cpu_baseline and world == 1:
            out["cpu_baseline"] = cpu_baseline(cfg, False)
        print(json.dumps(out), flush=True)
    if world > 1:
        torch.distributed.barrier()
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
