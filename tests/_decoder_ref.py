"""The transformer decoder written out from its definition, in a chosen precision (float64 by default), on the CPU.

ModRZTXDecoderLayer (tal/asr/models.py:488-528) with torch.nn.MultiheadAttention in eval mode, the tied factorised LM head
(models.py:218-247), the greedy pick of System.generate_unaligned (system.py:355-411) and the beam candidate selection of
System.generate (system.py:141-160).  Nothing here calls the library or the oracle: tests compare the kernels with it.

Layout is batch-major: tgt [B, U, E], memory [B, S, E].  Every function takes `dtype`; float64 is the reference, CPU
float32 is the same arithmetic at the kernels' precision and gives the error budget of a test (tests/test_gpu_decoder_kernels.py).
Weights come as a dict of the layer's state_dict names (numpy arrays or tensors)."""
import math

import numpy as np
import torch

F64 = torch.float64


def _t(x, dtype):
    if isinstance(x, torch.Tensor):
        return x.detach().to(device="cpu", dtype=dtype)
    return torch.as_tensor(np.asarray(x)).to(dtype)


def layer_params(layer):
    """state_dict of a ModRZTXDecoderLayer (any device) as CPU tensors."""
    return {k: v.detach().cpu() for k, v in layer.state_dict().items()}


def positional_encoding(max_len, d_model, dtype=F64):
    """PositionalEncoding's table pe [max_len, d_model] (tal/modules.py:45-51)."""
    pos = torch.arange(max_len, dtype=dtype).unsqueeze(1)
    div = torch.exp(torch.arange(0, d_model, 2, dtype=dtype) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(max_len, d_model, dtype=dtype)
    pe[:, 0::2] = torch.sin(pos * div)
    pe[:, 1::2] = torch.cos(pos * div)
    return pe


def causal_mask(n, dtype=F64):
    """Additive mask: -inf above the diagonal."""
    m = torch.zeros(n, n, dtype=dtype)
    return m.masked_fill(torch.triu(torch.ones(n, n, dtype=torch.bool), 1), float("-inf"))


def mha(query, key, w_in, b_in, w_out, b_out, nhead, attn_mask=None, kpm=None, dtype=F64):
    """Multi-head attention, key = value: query [B, U, E], key [B, S, E]; packed in-projection [3E, E], q scaled by hd^-0.5
    after its bias; additive attn_mask [U, S]; boolean key-padding mask [B, S] (True -> -inf).
    -> (out [B, U, E], per-head probabilities [B, H, U, S])."""
    q_in, k_in = _t(query, dtype), _t(key, dtype)
    B, U, E = q_in.shape
    S = k_in.shape[1]
    hd = E // nhead
    w, b = _t(w_in, dtype), _t(b_in, dtype)
    q = (q_in @ w[:E].T + b[:E]) * (float(hd) ** -0.5)
    k = k_in @ w[E:2 * E].T + b[E:2 * E]
    v = k_in @ w[2 * E:].T + b[2 * E:]
    q = q.reshape(B, U, nhead, hd).transpose(1, 2)
    k = k.reshape(B, S, nhead, hd).transpose(1, 2)
    v = v.reshape(B, S, nhead, hd).transpose(1, 2)
    scores = q @ k.transpose(-1, -2)
    if attn_mask is not None:
        scores = scores + _t(attn_mask, dtype).view(1, 1, U, S)
    if kpm is not None:
        scores = scores.masked_fill(_t(kpm, torch.bool).view(B, 1, 1, S), float("-inf"))
    probs = torch.softmax(scores, dim=-1)
    ctx = (probs @ v).transpose(1, 2).reshape(B, U, E)
    return ctx @ _t(w_out, dtype).T + _t(b_out, dtype), probs


def decoder_layer(tgt, memory, p, nhead, tgt_mask=None, kpm=None, dtype=F64):
    """ModRZTXDecoderLayer.forward: ReZero skips around self-attention, cross-attention and the ReLU FFN.
    -> (out [B, U, E], head-averaged cross-attention weights [B, U, S], per-head probabilities [B, H, U, S])."""
    x = _t(tgt, dtype)
    rw, rws = _t(p["resweight"], dtype).reshape(()), _t(p["resweight_src"], dtype).reshape(())
    a, _ = mha(x, x, p["self_attn.in_proj_weight"], p["self_attn.in_proj_bias"], p["self_attn.out_proj.weight"],
               p["self_attn.out_proj.bias"], nhead, attn_mask=tgt_mask, dtype=dtype)
    x = x + a * rw
    a, probs = mha(x, memory, p["multihead_attn.in_proj_weight"], p["multihead_attn.in_proj_bias"],
                   p["multihead_attn.out_proj.weight"], p["multihead_attn.out_proj.bias"], nhead, kpm=kpm, dtype=dtype)
    x = x + a * rws
    h = torch.relu(x @ _t(p["linear1.weight"], dtype).T + _t(p["linear1.bias"], dtype))
    h = h @ _t(p["linear2.weight"], dtype).T + _t(p["linear2.bias"], dtype)
    return x + h * rw, probs.mean(dim=1), probs


def decoder_stack(tgt, memory, layers, nhead, tgt_mask=None, kpm=None, dtype=F64):
    """Layers in sequence (nn.TransformerDecoder, norm=None) -> (out, [head-averaged weights per layer])."""
    x, avgs = tgt, []
    for p in layers:
        x, avg, _ = decoder_layer(x, memory, p, nhead, tgt_mask, kpm, dtype)
        avgs.append(avg)
    return x, avgs


def embed_tokens(tokens, emb, proj, pe, dtype=F64):
    """embedding -> embedding_proj (proj [E, E0] or None) -> + pe[:U]: tokens [B, U] -> [B, U, E]."""
    tok = torch.as_tensor(np.asarray(tokens), dtype=torch.long)
    e = _t(emb, dtype)[tok]
    if proj is not None:
        e = e @ _t(proj, dtype).T
    return e + _t(pe, dtype)[: tok.shape[-1]]


def lm_logits(h, emb, proj, dtype=F64):
    """Tied factorised LM head: F.linear(F.linear(h, proj^T), emb) (models.py:243-246)."""
    x = _t(h, dtype)
    if proj is not None:
        x = x @ _t(proj, dtype)
    return x @ _t(emb, dtype).T


def greedy_step(tokens, memory, kpm, layers, nhead, emb, proj, pe, pick_bias=None, dtype=F64):
    """One step of the greedy loop on a window: prefix tokens [U], memory [S, E], kpm [S] bool or None.
    -> (scores [V] = last row's logits + pick_bias, attention row [S]: the last row's cross-attention averaged over heads,
    then over layers in layer order).  The pick is arg max of log_softmax(logits) + bias = arg max of the scores."""
    x = embed_tokens(np.asarray(tokens)[None], emb, proj, pe, dtype)
    km = None if kpm is None else _t(kpm, torch.bool)[None]
    h, avgs = decoder_stack(x, _t(memory, dtype)[None], layers, nhead, kpm=km, dtype=dtype)
    logits = lm_logits(h[0, -1], emb, proj, dtype)
    if pick_bias is not None:
        logits = logits + _t(pick_bias, dtype)
    row = avgs[0][0, -1]
    for a in avgs[1:]:
        row = row + a[0, -1]
    return logits, row / len(avgs)


def greedy_pick(scores):
    """arg max, the lowest index on ties (torch.argmax)."""
    return int(np.argmax(np.asarray(scores)))


def beam_topk(logprobs, row_score, row_done, k):
    """System.generate's candidate selection: logprobs [B, beam, V] + row_score [B, beam] (None: 0), rows with row_done
    [B, beam] set -> -inf, then per batch item the top k of the beam x V flat candidates, values descending, the lowest flat
    index first on ties.  -> (values [B, k], flat indices [B, k])."""
    lp = np.asarray(logprobs, dtype=np.float64)
    B, nb, V = lp.shape
    tot = lp + (0.0 if row_score is None else np.asarray(row_score, dtype=np.float64)[:, :, None])
    if row_done is not None:
        tot = np.where(np.asarray(row_done, dtype=bool)[:, :, None], -np.inf, tot)
    flat = tot.reshape(B, nb * V)
    idx = np.arange(nb * V)
    vals, ids = np.empty((B, k)), np.empty((B, k), dtype=np.int64)
    for b in range(B):
        order = np.lexsort((idx, -flat[b]))[:k]          # (primary key last: value descending, then index ascending)
        vals[b], ids[b] = flat[b, order], order
    return vals, ids
