"""Plain restatement of the RNN language model for the tests: table lookup, L-layer LSTM (gate order i, f, g, o; two biases),
Linear, LayerNorm, LeakyReLU(0.01), Linear.  Default float64 - the yardstick of tests/test_rnnlm_gpu.py, itself checked against a
torch.nn.Embedding -> torch.nn.LSTM -> Linear -> LayerNorm -> LeakyReLU -> Linear chain in tests/test_rnnlm_cpu.py.  The same code in
float32, for bf16 operands with h and the activations rounded to bf16 where the kernels store them, is the FLOOR emulation: what the
number formats alone cost.  Nothing here calls the code under test.

Parameters travel as a dict under the model's state-dict names (KEYS)."""
import torch

from tests._lstm_ref import bf16_round


def keys(L):
    ks = ["embedding.Embedding.weight"]
    for k in range(L):
        ks += [f"rnn.rnn.weight_ih_l{k}", f"rnn.rnn.weight_hh_l{k}", f"rnn.rnn.bias_ih_l{k}", f"rnn.rnn.bias_hh_l{k}"]
    return ks + ["dnn.linear.w.weight", "dnn.linear.w.bias", "dnn.norm.norm.weight", "dnn.norm.norm.bias", "out.w.weight", "out.w.bias"]


def shapes(V, E, H, L, D):
    s = {"embedding.Embedding.weight": (V, E)}
    for k in range(L):
        s.update({f"rnn.rnn.weight_ih_l{k}": (4 * H, E if k == 0 else H), f"rnn.rnn.weight_hh_l{k}": (4 * H, H),
                  f"rnn.rnn.bias_ih_l{k}": (4 * H,), f"rnn.rnn.bias_hh_l{k}": (4 * H,)})
    s.update({"dnn.linear.w.weight": (D, H), "dnn.linear.w.bias": (D,), "dnn.norm.norm.weight": (D,), "dnn.norm.norm.bias": (D,),
              "out.w.weight": (V, D), "out.w.bias": (V,)})
    return s


def make_params(V, E, H, L, D, seed, wide=True):
    """Random parameters.  wide: biases and W_ih from +-0.5 so that every gate matters; a NON-zero row 0 of the table."""
    g = torch.Generator().manual_seed(seed)
    u = lambda shape, a: (torch.rand(shape, generator=g) * 2 - 1) * a
    sd = {}
    for name, shape in shapes(V, E, H, L, D).items():
        if name.startswith("embedding"):
            sd[name] = torch.randn(shape, generator=g)
        elif "weight_ih" in name or "rnn.rnn.bias" in name:
            sd[name] = u(shape, 0.5 if wide else H ** -0.5)
        elif "weight_hh" in name:
            sd[name] = u(shape, H ** -0.5)
        elif name == "dnn.norm.norm.weight":
            sd[name] = 1.0 + u(shape, 0.3)
        elif name.endswith("bias"):
            sd[name] = u(shape, 0.3)
        else:
            sd[name] = u(shape, shape[1] ** -0.5)
    return sd


def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One step: x (B, I), h / c (B, H) -> (h', c')."""
    H = h.shape[1]
    z = (b_ih + b_hh) + x @ w_ih.t() + h @ w_hh.t()
    i, f, g, o = torch.sigmoid(z[:, :H]), torch.sigmoid(z[:, H:2 * H]), torch.tanh(z[:, 2 * H:3 * H]), torch.sigmoid(z[:, 3 * H:])
    c = f * c + i * g
    return o * torch.tanh(c), c


def lookup(table, tokens):
    """table[tokens] as stored; a token outside the table reads as a zero row."""
    ok = (tokens >= 0) & (tokens < table.shape[0])
    return table[tokens.clamp(0, table.shape[0] - 1).long()] * ok.unsqueeze(-1).to(table.dtype)


def head(y, sd, rnd=None, slope=0.01, eps=1e-5):
    r = rnd or (lambda t: t)
    z = r(y @ sd["dnn.linear.w.weight"].t() + sd["dnn.linear.w.bias"])
    mu, var = z.mean(-1, keepdim=True), z.var(-1, unbiased=False, keepdim=True)
    a = (z - mu) / torch.sqrt(var + eps) * sd["dnn.norm.norm.weight"] + sd["dnn.norm.norm.bias"]
    a = r(torch.where(a >= 0, a, slope * a))
    return r(a @ sd["out.w.weight"].t() + sd["out.w.bias"])


def run(sd, tokens, L, hx=None, dtype=torch.float64, rnd=None):
    """tokens (B, U) -> dict(logits (B, U, V), hn (L, B, H), cn (L, B, H), y (B, U, H) the top layer's output).  rnd (a function or None)
    is applied to the table rows as read, to h where it is stored / fed back and to the head's stored activations and logits."""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    B, U = tokens.shape
    H = sd["rnn.rnn.weight_hh_l0"].shape[1]
    r = rnd or (lambda t: t)
    x = lookup(sd["embedding.Embedding.weight"], tokens)
    hn, cn = [], []
    for k in range(L):
        p = [sd[f"rnn.rnn.{n}_l{k}"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        h = r(hx[0][k].to(dtype)) if hx is not None else torch.zeros(B, H, dtype=dtype)
        c = hx[1][k].to(dtype) if hx is not None else torch.zeros(B, H, dtype=dtype)
        ys = []
        for u in range(U):
            h, c = lstm_cell(x[:, u], h, c, *p)
            h = r(h)
            ys.append(h)
        x = torch.stack(ys, 1)
        hn.append(h)
        cn.append(c)
    return {"logits": head(x, sd, rnd), "hn": torch.stack(hn), "cn": torch.stack(cn), "y": x}


def rounded(sd, operand_dtype):
    """The parameters as the kernels see them: matrices and the table rounded to the operand dtype, vectors (biases, LayerNorm) fp32."""
    return {k: (v.to(operand_dtype).double() if v.dim() == 2 else v.float().double()) for k, v in sd.items()}


def floor_and_ref(operand_dtype, sd, tokens, L, hx=None):
    """(fp64 reference, floor emulation) on the dtype-rounded parameters: the emulation is `run` in float32, for bf16 operands with
    h, the head's activations and the logits rounded to bf16 where the kernels store them."""
    sdr = rounded(sd, operand_dtype)
    ref = run(sdr, tokens, L, hx, torch.float64)
    emu = run(sdr, tokens, L, hx, torch.float32, bf16_round if operand_dtype == torch.bfloat16 else None)
    return ref, emu
