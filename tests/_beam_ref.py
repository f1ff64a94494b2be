"""Numpy model of the bookkeeping of System.generate's beam loop (tal/asr/system.py:141-219), the yardstick for the
device-resident search (tal_beam_ctx, csrc/beam.hip): per step it takes the (values, flat indices) of a selection and keeps
tokens, scores, `done`, the finish records, the parent rows and the step at which the loop stops.

Speaker logits are kept TWICE: re-threaded every step with index_select + cat as the reference does (`spk_embeds`), and as
per-step rows with their parent rows, read back along the chain by `gather` -- the form the device keeps.  The CPU tests
hold the two against each other; the GPU tests hold the device against the first.

`topk_ref` is the selection itself in tal_beam_topk's order (value descending, lowest flat index on ties, NaN last by index and
reported as -inf), for small shapes."""
import numpy as np


def topk_ref(logprobs, scores, done, B, cur_beam, k):
    """logprobs float32 [B * cur_beam, V]; scores float32 [B * cur_beam]; done bool [B * cur_beam] or None -> (vals [B, k], idx [B, k])."""
    V = logprobs.shape[1]
    total = (logprobs.astype(np.float32) + scores.astype(np.float32)[:, None]).astype(np.float32)
    if done is not None:
        total[np.asarray(done, dtype=bool)] = -np.inf
    total = total.reshape(B, cur_beam * V)
    vals = np.empty((B, k), dtype=np.float32)
    idx = np.empty((B, k), dtype=np.int64)
    for b in range(B):
        row = total[b]
        nan = np.isnan(row)
        # non-NaN first by (-value, index); then the NaN ones by index
        order = np.lexsort((np.arange(row.size), np.where(nan, 0.0, -row.astype(np.float64)), nan))
        pick = order[:k]
        idx[b] = pick
        vals[b] = np.where(nan[pick], -np.inf, row[pick])
    return vals, idx


class BeamRef:
    def __init__(self, generated, beam, V, terminate_token=None, num_speakers=0):
        generated = np.asarray(generated, dtype=np.int64)
        self.B, self.L0 = generated.shape
        self.beam, self.V, self.terminate, self.ns = beam, V, terminate_token, num_speakers
        self.R = self.B * beam
        self.tokens = np.repeat(generated, beam, axis=0)          # [R, L0 + step] (system.py:165-166)
        self.scores = np.zeros(self.R, dtype=np.float32)
        self.done = np.zeros(self.R, dtype=bool)
        self.records = []                                         # dicts: slot, step, row, score (float32), spk
        self.step = 0
        self.stopped = False
        self.spk_embeds = None                                    # [R, step, ns], re-threaded (system.py:184-196)
        self.spk_rows = []                                        # per step [R, ns] as stored
        self.parents = []                                         # per step int [R]

    @property
    def cur_beam(self):
        return 1 if self.step == 0 and self.beam > 1 else self.beam

    def mask(self):
        """The done mask of the next selection: applied only once cur_beam == beam."""
        return self.done.copy() if self.cur_beam == self.beam else None

    def advance(self, vals, idx, spk=None):
        """One step's bookkeeping on the selection (vals [B, beam] float32, idx [B, beam] flat indices); spk [rows of this step, ns].
        After the loop has stopped (every slot done: the reference `break`s) nothing changes any more."""
        if self.stopped:
            return
        vals = np.asarray(vals, dtype=np.float32).reshape(self.B, self.beam)
        idx = np.asarray(idx, dtype=np.int64).reshape(self.B, self.beam)
        rep = self.beam // self.cur_beam
        best_tokens = idx % self.V
        best_beams = idx // self.V
        src = (np.arange(self.B)[:, None] * self.beam + best_beams).reshape(-1)
        self.tokens = np.concatenate([self.tokens[src], best_tokens.reshape(-1, 1)], axis=1)
        self.scores = vals.reshape(-1).copy()
        if spk is not None:
            spk = np.asarray(spk, dtype=np.float32)
            if self.spk_embeds is None:
                self.spk_embeds = np.repeat(spk[:, None, :], rep, axis=0)
            else:
                self.spk_embeds = np.concatenate([self.spk_embeds[src], spk[:, None, :]], axis=1)
            self.spk_rows.append(np.repeat(spk, rep, axis=0))
            self.parents.append(src.astype(np.int64))
        if self.terminate is not None:
            for slot in np.nonzero(best_tokens.reshape(-1) == self.terminate)[0].tolist():
                if not self.done[slot]:
                    self.records.append({"slot": slot, "step": self.step, "row": self.tokens[slot].copy(), "score": self.scores[slot],
                                         "spk": None if self.spk_embeds is None else self.spk_embeds[slot].copy()})
                    self.done[slot] = True
        self.step += 1
        if self.done.sum() >= self.R:
            self.stopped = True

    def gather(self, slot, step):
        """Speaker history [step + 1, ns] of the hypothesis in `slot` after step `step`, along the parent rows."""
        out = np.empty((step + 1, self.ns), dtype=np.float32)
        r = slot
        for s in range(step, -1, -1):
            out[s] = self.spk_rows[s][r]
            r = int(self.parents[s][r])
        return out

    def record_arrays(self):
        """(rec_step [R] with -1 for none, rec_score [R], rows: {slot: token row}) -- the device's form of the records."""
        rec_step = np.full(self.R, -1, dtype=np.int32)
        rec_score = np.zeros(self.R, dtype=np.float32)
        rows = {}
        for r in self.records:
            rec_step[r["slot"]] = r["step"]
            rec_score[r["slot"]] = r["score"]
            rows[r["slot"]] = r["row"]
        return rec_step, rec_score, rows
