"""Which gradient buckets of a data-parallel FlagStep (immtsf.train) share a wire image, a counting flag and a collective, and in which
order the communication stream waits for them.  Host bookkeeping only: nothing here launches but the `emit` the engine supplies."""


def runs(ranges):
    """contiguous runs of (lo, hi) ranges (sorted by lo; empty ones dropped)"""
    out = []
    for lo, hi in sorted(r for r in ranges if r[1] > r[0]):
        if out and out[-1][1] == lo:
            out[-1] = (out[-1][0], hi)
        else:
            out.append((lo, hi))
    return out


class Announcer:
    """ranges: every bucket's (lo, hi) in the flat buffer.  emit(k, lo, hi) -> flag address: announce flat[lo:hi] as the k-th segment,
    on the current stream.  An EMPTY bucket counts as announced and appears in no segment."""

    def __init__(self, ranges, emit, merge_adjacent=True, capacity=24):
        self.ranges, self.emit, self.merge_adjacent, self.capacity = list(ranges), emit, merge_adjacent, capacity
        self.branch = "T"               # "T" | "B" | "P" | "J": the engine says which branch it is capturing
        self.segments = []              # [dict(flag, flags, lo, hi, buckets, branch)], in announcement order
        self._announced, self._bursts = set(), {}

    def _emit_runs(self, members):
        members = sorted(members, key=lambda b: self.ranges[b])
        for lo, hi in runs([self.ranges[b] for b in members]):
            if len(self.segments) >= self.capacity:
                raise RuntimeError(f"FlagStep: more than {self.capacity} announced buckets")
            flag = self.emit(len(self.segments), lo, hi)
            inside = tuple(b for b in members if lo <= self.ranges[b][0] < self.ranges[b][1] <= hi)
            self.segments.append({"flag": flag, "flags": [flag], "lo": lo, "hi": hi, "buckets": inside, "branch": self.branch * len(inside)})

    def announce(self, bi, burst=None):
        """bucket `bi` is final.  burst = (token, i, cnt): hooks fired back to back (the buckets complete at the same moment): its members
        that are neighbours in the flat buffer get ONE wire image, ONE flag and ONE collective -- emitted when its last member reports"""
        if bi in self._announced:
            return
        self._announced.add(bi)
        if burst is None or not self.merge_adjacent:
            self._emit_runs([bi])
            return
        token, i, cnt = burst
        self._bursts.setdefault(id(token), []).append(bi)
        if i + 1 >= cnt:
            self._emit_runs(self._bursts.pop(id(token)))

    def finish(self):
        """behind the join everything is complete: the bursts still open (their last member was announced before them), then what
        nobody announced, as contiguous runs"""
        self.branch = "J"
        rest = [bi for bi in range(len(self.ranges)) if bi not in self._announced]
        self._announced.update(rest)
        for members in [self._bursts.pop(k) for k in list(self._bursts)] + [rest]:
            self._emit_runs(members)


def static_order(segments):
    """the communication order before any measurement: the text side's segments but its last, the parameter branch's, the text side's
    last, the backbone's, the join's; the SAME on every rank (FlagStep.calibrate_comm_order replaces it by the measured order)"""
    by = {c: [g for g in segments if g["branch"][0] == c] for c in "TPBJ"}
    return by["T"][:-1] + by["P"] + by["T"][-1:] + by["B"] + by["J"]


def merge_tail(segs, merge_tail_us):
    """segs: segments with `done_us`, in completion order.  The ones that complete within `merge_tail_us` of the LAST one, when they
    are one contiguous range of the flat buffer, go out as ONE collective behind one wait on all their flags: every collective in the
    exposed tail costs its full latency (three collectives behind the last flag: +37 us at one rank, ~3 x the RCCL latency at eight);
    an earlier bucket keeps its own"""
    tail = [g for g in segs if segs[-1]["done_us"] - g["done_us"] <= merge_tail_us]
    by_lo = sorted(tail, key=lambda g: g["lo"])
    if len(tail) < 2 or sum(g["hi"] - g["lo"] for g in tail) != by_lo[-1]["hi"] - by_lo[0]["lo"]:
        return segs
    merged = dict(tail[-1], flags=[f for g in tail for f in g["flags"]], lo=by_lo[0]["lo"], hi=by_lo[-1]["hi"],
                  buckets=tuple(b for g in by_lo for b in g["buckets"]), branch="".join(g["branch"] for g in by_lo))
    return segs[:len(segs) - len(tail)] + [merged]
