"""Speaker turns as text: seconds and RTTM lines.  Host text only -- the turns come from ops.speaker_turns /
SDModel.speaker_turns (device tensors); turns_to_seconds copies one item's few turns to the host."""

FRAME_STRIDE_S = 0.08      # one encoder frame: 10 ms log-mel hop x the TDS encoder's stride of 8


def turns_to_seconds(result, item=0, stride=FRAME_STRIDE_S):
    """The turns of item `item` of a SpeakerTurns result -> [(start_s, end_s, label, purity)].  Frame f covers
    [f * stride, (f + 1) * stride), so a turn of frames [start, end) covers [start * stride, end * stride)."""
    off = result.offsets[item:item + 2].tolist()
    if len(off) != 2:
        raise IndexError("turns_to_seconds: item %d of %d" % (item, result.offsets.numel() - 1))
    a, b = off
    cols = [t[a:b].tolist() for t in (result.start, result.end, result.label, result.purity)]
    return [(s * stride, e * stride, int(lab), int(p)) for s, e, lab, p in zip(*cols)]


def write_rttm(fh, uri, turns):
    """One standard RTTM line per turn: SPEAKER <uri> 1 <start> <duration> <NA> <NA> <label> <NA> <NA>, seconds with three
    decimals.  turns: (start_s, end_s, label[, ...]) tuples, e.g. turns_to_seconds' output.  Returns the number of lines."""
    if not uri or any(c.isspace() for c in str(uri)):
        raise ValueError("write_rttm: the uri %r must be a non-empty token without white space" % (uri,))
    n = 0
    for turn in turns:
        start, end, label = turn[0], turn[1], turn[2]
        if end < start:
            raise ValueError("write_rttm: turn (%r, %r) ends before it starts" % (start, end))
        fh.write("SPEAKER %s 1 %.3f %.3f <NA> <NA> %s <NA> <NA>\n" % (uri, start, end - start, label))
        n += 1
    return n


def read_rttm(fh):
    """The SPEAKER lines of an RTTM file -> [(uri, start_s, end_s, label)] (labels as written: strings)."""
    out = []
    for line in fh:
        parts = line.split()
        if not parts or parts[0] != "SPEAKER":
            continue
        if len(parts) < 8:
            raise ValueError("read_rttm: short SPEAKER line %r" % line)
        start, dur = float(parts[3]), float(parts[4])
        out.append((parts[1], start, start + dur, parts[7]))
    return out
