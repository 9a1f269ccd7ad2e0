"""Restatement of TransformerLM, written from the formulas of speechbrain's Transformer.py (NormalizedEmbedding +
positional rows, get_key_padding_mask, get_lookahead_mask, TransformerEncoderLayer with regularMHA in both normalize_before orders,
TransformerEncoder's final LayerNorm) and upstream's output head (Linear, LayerNorm, Linear), over ONE parameter dict with the
package's state_dict keys, in the two arithmetic flavours of tests/_decoder_ref.py (impl="f64": float64 on the CPU, the yardstick;
impl="aten": the ATen chain at the tensors' own dtype and device, whose error against float64 sets the bar).  Then the LM's share of
the beam search's scores, and a scorer that drives tests/_ctc_prefix_ref.search with it.

The state_dict keys: ``encoder.*`` are those of the reference's own TransformerEncoder(attention_type="regularMHA"), recorded in
tests/golden/transformerlm_state_keys.json from that class instantiated through tests/golden/sb_standin (whose MultiheadAttention
stand-in was given upstream's layout, ``.att`` = torch.nn.MultiheadAttention, for that run); ``custom_src_module.*``,
``output_proj.*`` and ``positional_encoding.pe`` are stated from upstream's TransformerLM.py, which is not part of the reference tree."""
import torch
import torch.nn.functional as TF

from tests import _decoder_ref as DR

NEG_INF = float("-inf")
TABLE, PE = "custom_src_module.emb.Embedding.weight", "positional_encoding.pe"


def outer_keys(d, vocab, max_length):
    """The three outer groups, as upstream's TransformerLM registers them: name -> shape."""
    return {TABLE: (vocab, d), PE: (1, max_length, d),
            "output_proj.layers.0.w.weight": (d, d), "output_proj.layers.0.w.bias": (d,),
            "output_proj.layers.1.norm.weight": (d,), "output_proj.layers.1.norm.bias": (d,),
            "output_proj.layers.2.w.weight": (vocab, d), "output_proj.layers.2.w.bias": (vocab,)}


def encoder_layer(x, P, pfx, nhead, act, pre, pad, impl):
    """One TransformerEncoderLayer (eps 1e-6), causal, key padding `pad` (B, U) bool or None."""
    d = x.shape[-1]

    def ln(t, n):
        return TF.layer_norm(t, (d,), P[f"{pfx}{n}.norm.weight"], P[f"{pfx}{n}.norm.bias"], 1e-6)
    a = f"{pfx}self_att.att."
    t1 = ln(x, "norm1") if pre else x
    t2, _ = DR._mha(impl, t1, t1, t1, P[a + "in_proj_weight"], P[a + "in_proj_bias"], P[a + "out_proj.weight"], P[a + "out_proj.bias"],
                    nhead, None, pad, True)
    x = x + t2
    if not pre:
        x = ln(x, "norm1")
    t1 = ln(x, "norm2") if pre else x
    h = DR._act(act, TF.linear(t1, P[pfx + "pos_ffn.ffn.0.weight"], P[pfx + "pos_ffn.ffn.0.bias"]))
    x = x + TF.linear(h, P[pfx + "pos_ffn.ffn.3.weight"], P[pfx + "pos_ffn.ffn.3.bias"])
    if not pre:
        x = ln(x, "norm2")
    return x


def head(x, P):
    """encoder.norm, then output_proj: Linear, LayerNorm (eps 1e-6), Linear; no activation."""
    d = x.shape[-1]
    x = TF.layer_norm(x, (d,), P["encoder.norm.norm.weight"], P["encoder.norm.norm.bias"], 1e-6)
    x = TF.linear(x, P["output_proj.layers.0.w.weight"], P["output_proj.layers.0.w.bias"])
    x = TF.layer_norm(x, (d,), P["output_proj.layers.1.norm.weight"], P["output_proj.layers.1.norm.bias"], 1e-6)
    return TF.linear(x, P["output_proj.layers.2.w.weight"], P["output_proj.layers.2.w.bias"])


def lm(tokens, P, n_layers, nhead, act, pre, impl="f64", pad_idx=0, mask_pad=True, dtype=torch.float64):
    """tokens (B, U) -> logits (B, U, V).  mask_pad=False: no key-padding mask, what the cached step computes."""
    x = DR.embed(tokens, P[TABLE], P[PE][0]).to(dtype)
    pad = (tokens == pad_idx) if mask_pad else None
    for i in range(n_layers):
        x = encoder_layer(x, P, f"encoder.layers.{i}.", nhead, act, pre, pad, impl)
    return head(x, P)


def lm_score(z, temperature, weight):
    """weight * log_softmax(z / temperature) in float64; a row holding a NaN or no number: -inf everywhere."""
    z = z.detach().double().cpu()
    out = weight * torch.log_softmax(z / temperature, -1)
    bad = torch.isnan(z).any(-1) | (z == NEG_INF).all(-1)
    out[bad] = NEG_INF
    return out


class JointScorer:
    """What tests/_ctc_prefix_ref.search asks of a scorer (extra / advance / lp), for the LM alone or behind a
    tests/_ctc_prefix_ref.PrefixScorer: extra = [the CTC scorer's extra] + w_lm log_softmax(LM logits of the row's whole prefix /
    t_lm)[v], in `dtype`; rows that are dead or of a done utterance score -inf.  lm_fn(prefixes (B W, n + 1) int64 on the CPU) ->
    logits (B W, n + 1, V), the LM run with no key-padding mask (the cached step's definition)."""

    def __init__(self, lm_fn, B, W, V, bos, eos, w_lm, t_lm, ctc=None, dtype=torch.float64):
        self.lm_fn, self.B, self.W, self.V, self.bos, self.eos, self.w_lm, self.t_lm, self.ctc, self.dtype = lm_fn, B, W, V, bos, eos, w_lm, t_lm, ctc, dtype

    def extra(self, beam, logits):
        B, W, V = self.B, self.W, self.V
        z = logits.detach().to("cpu", self.dtype).view(B, W, V)
        self.lp = torch.log_softmax(z / beam.T, -1)
        n = max(beam.n[b] for b in range(B) if not beam.done[b])
        prefixes = torch.tensor([([self.bos] + beam.tokens[b][i] + [self.eos] * n)[:n + 1] for b in range(B) for i in range(W)], dtype=torch.int64)
        prefixes[(prefixes < 0) | (prefixes >= V)] = 0
        lz = self.lm_fn(prefixes)[:, -1].detach().to("cpu", self.dtype)
        self.lmlp = torch.log_softmax(lz / self.t_lm, -1)
        if self.ctc is not None:
            base = self.ctc.extra(beam, logits).to(self.dtype)
        else:
            base = torch.full((B * W, V), NEG_INF, dtype=self.dtype)
            for b in range(B):
                for i in range(W):
                    if not beam.done[b] and beam.alive(b, i):
                        base[b * W + i] = 0.0
        return base + self.w_lm * self.lmlp

    def advance(self, beam, was_done, stepped):
        if self.ctc is not None:
            self.ctc.advance(beam, was_done, stepped)
