"""A store of arrays and a sequence of calls on it, for tests/test_gpu_context_history.py: what one long-lived context must return,
write and leave behind, call after call.  Pure Python and numpy: neither torch nor the library is loaded here, so the sequence and
the model can be checked without a GPU (tests/test_context_history_cpu.py).

THE MODEL (class Model) holds every array of the store as a numpy uint8 array; arrays are replaced, never modified in place, so an
operation can hand out the arrays as they were before it.  Three groups of frames, a call stays within one group:

  A  bytesoftype 4, 6 frames: [0] 300 superblocks (many-frame calls walk it in parallel, the others in one launch), [1] [2] large,
     [3] [4] small, [5] the page: an empty array (the 8-byte frame), which only the many-frame calls and `batch` look at;
  B  bytesoftype 8, 4 frames: [0] [1] large, [2] [3] small;
  C  bytesoftype 3, 4 frames: the same.

Slots [1] and [3] of A, [0] and [2] of B and C hold noise (stored as copies), the others compressible or mixed data; an array that
`compress` replaces keeps the kind and the regime of its slot.  The page is filled by `append_batch` when it is empty, and `batch`
on group A starts a new, empty one.

Every method of the model takes a Step and returns a dict: "before" / "after" (arrays by frame number), "error" (the code a
failing call must return; the model is then unchanged) and what the call is made of (rows, ranges, sources, expected rows).

THE SEQUENCE (sequence) is an Eulerian circuit (Hierholzer, fixed start, the order of the edges shuffled by the seed) of the
complete directed graph with loops on the 14 classes: 197 steps, every ordered pair (previous class, class) exactly once.  A seeded
generator gives every step its regime, group and frame.  A sequence is a list of (class, regime, group, frame): for `fail` the
fourth entry names the failing call, for calls over a whole group it is -1.  steps_of derives the rest from the list alone -- the
index form, the stream -- so a prefix of the list replays the same calls.

INDEX FORMS.  "own": the context's pointer (stenos_hip_last_index / stenos_hip_last_frames_index), scheduled wherever the step
before leaves one that include/stenos_hip.h calls valid for the very frames of this step (the generator then puts the step on those
frames); elsewhere "null" and "copy" (true entries in a tensor of the caller's) take turns per class.

FAILING CALLS.  There are nine; the pair (fail, X) occurs once for every X, so only six `fail` steps are followed by a call of
the family of what failed, two per family -- FOLLOWED_BY says which -- and the other eight steps rotate through the rest."""
from collections import namedtuple

import numpy as np

from test_gpu_ranges import _data, _mixed_data, _sb, range_set

SEED = 24
CLASSES = ("compress", "compress_async", "batch", "decompress", "ranges", "gather", "gather_batch", "update", "update_batch", "append", "append_batch", "index", "host",
           "fail")
SINGLE_INDEX = ("decompress", "ranges", "gather", "update", "append")
MANY_INDEX = ("gather_batch", "update_batch", "append_batch")
GROUPS = {"A": (4, 6), "B": (8, 4), "C": (3, 4)}  # bytesoftype, frames
BIG, PAGE = 0, 5  # of group A
BIG_SUPERBLOCKS = 300
SLOTS = {"A": {"large": (0, 1, 2), "small": (3, 4)}, "B": {"large": (0, 1), "small": (2, 3)}, "C": {"large": (0, 1), "small": (2, 3)}}
NOISE = {"A": (1, 3), "B": (0, 2), "C": (0, 2)}
FAMILIES = {"gather": ("gather", "gather_batch"), "update": ("update", "update_batch"), "append": ("append", "append_batch")}
FAILS = ("gather_bad_row", "update_bad_row", "gather_batch_bad_pair", "update_batch_bad_pair", "update_dst_overflow", "append_dst_overflow", "gather_damaged",
         "append_damaged", "append_batch_damaged")
FAIL_FAMILY = {"gather_bad_row": "gather", "gather_batch_bad_pair": "gather", "gather_damaged": "gather", "update_bad_row": "update", "update_batch_bad_pair": "update",
               "update_dst_overflow": "update", "append_dst_overflow": "append", "append_damaged": "append", "append_batch_damaged": "append"}
FOLLOWED_BY = {"gather": "gather_damaged", "gather_batch": "gather_batch_bad_pair", "update": "update_dst_overflow", "update_batch": "update_batch_bad_pair",
               "append": "append_damaged", "append_batch": "append_batch_damaged"}
E = lambda k: (1 << 64) - k  # noqa: E731
INVALID_PARAMETER, SRC_OVERFLOW, INVALID_INPUT, DST_OVERFLOW = E(9), E(2), E(4), E(6)

Step = namedtuple("Step", "i cls prev regime group frame form stream kind")


def slot_regime(group, frame):
    return next((r for r, slots in SLOTS[group].items() if frame in slots), None)


class Tracker:
    """what a sequence so far leaves in the context: ("single", group, frame), ("many", group) or None; and the per-class turns"""

    def __init__(self):
        self.left, self.turns, self.steps = None, {}, []

    def wanted(self, cls, group, frame):
        return ("single", group, frame) if cls in SINGLE_INDEX else ("many", group) if cls in MANY_INDEX else None

    def push(self, spec):
        cls, regime, group, frame = spec
        form = None
        if cls in SINGLE_INDEX or cls in MANY_INDEX:
            if self.left is not None and self.left == self.wanted(cls, group, frame):
                form = "own"
            else:
                k = self.turns.get(cls, 0)
                self.turns[cls] = k + 1
                form = ("null", "copy")[k % 2]
        i = len(self.steps)
        step = Step(i, cls, self.steps[-1].cls if self.steps else None, regime, group, frame if cls != "fail" else -1, form, i % 3, frame if cls == "fail" else None)
        self.steps.append(step)
        if cls in ("compress", "compress_async", "update", "append"):
            self.left = ("single", group, frame)
        elif cls in ("index", "update_batch", "append_batch"):
            self.left = ("many", group)
        elif not (cls in ("ranges", "gather", "gather_batch") and form == "own"):  # (these leave the context's index as it is)
            self.left = None
        return step


def steps_of(specs):
    t = Tracker()
    for spec in specs:
        t.push(tuple(spec))
    return t.steps


def euler_classes(seed=SEED):
    rng = np.random.default_rng([seed, 1])
    out = {c: [CLASSES[k] for k in rng.permutation(len(CLASSES))] for c in CLASSES}
    stack, circuit = [CLASSES[0]], []
    while stack:
        if out[stack[-1]]:
            stack.append(out[stack[-1]].pop())
        else:
            circuit.append(stack.pop())
    return circuit[::-1]


def sequence(seed=SEED):
    classes = euler_classes(seed)
    rng = np.random.default_rng([seed, 2])
    t = Tracker()
    specs = []
    rest = [k for k in FAILS if k not in FOLLOWED_BY.values()] + list(FAILS)
    nrest = 0
    behind_large = dict.fromkeys(CLASSES, 0)
    for i, cls in enumerate(classes):
        # small behind large as often as it takes: every class three times; then large and small in turn, one step in five at random
        prev_large = bool(specs) and specs[-1][1] == "large"
        now, then = (3 - behind_large[cls] if prev_large else 0), (3 - behind_large[classes[i + 1]] if i + 1 < len(classes) else 0)
        if max(now, then) > 0:
            regime = "small" if now > 0 and now >= then else "large"
        else:
            regime = ("small" if prev_large else "large") if rng.random() < 0.8 else ("large", "small")[int(rng.integers(0, 2))]
        group = "AABBCC"[int(rng.integers(0, 6))] if cls not in MANY_INDEX + ("index", "batch") else "AAABBC"[int(rng.integers(0, 6))]
        pick = int(rng.integers(0, 6))
        frame = -1
        if cls == "fail":
            nxt = classes[i + 1] if i + 1 < len(classes) else None
            if nxt in FOLLOWED_BY:
                frame = FOLLOWED_BY[nxt]
            else:
                frame = rest[nrest % len(rest)]
                nrest += 1
        elif cls in SINGLE_INDEX and t.left and t.left[0] == "single":
            group, frame = t.left[1], t.left[2]
            regime = slot_regime(group, frame)
        elif cls in MANY_INDEX and t.left and t.left[0] == "many":
            group = t.left[1]
        elif cls in SINGLE_INDEX + ("index", "compress", "compress_async"):
            slots = [s for s in SLOTS[group][regime] if not (cls.startswith("compress") and group == "A" and s == BIG)]
            frame = slots[pick % len(slots)]
        behind_large[cls] += regime == "small" and bool(specs) and specs[-1][1] == "large"
        specs.append((cls, regime, group, frame))
        t.push(specs[-1])
    return specs


def _rows_of(arr, rows, rb):
    col = np.arange(rb, dtype=np.int64)
    return arr[(np.asarray(rows, dtype=np.int64) * rb)[:, None] + col] if len(rows) else np.zeros((0, rb), dtype=np.uint8)


def _overlay(arr, rows, rb, src_rows):
    out = arr.copy()
    if len(rows):
        out[(np.asarray(rows, dtype=np.int64) * rb)[:, None] + np.arange(rb, dtype=np.int64)] = src_rows
    return out


class Model:
    def __init__(self):
        self.arrays = {g: [None] * n for g, (_, n) in GROUPS.items()}
        self.turn = self.small_turn = 0
        for g, (T, n) in GROUPS.items():
            sb = _sb(T)
            small = {"A": (sb + 1, 127), "B": (sb - 1, sb + 256 * T + 37), "C": (128, sb)}[g]
            for f in range(n):
                if g == "A" and f == BIG:
                    self.arrays[g][f] = _mixed_data(T, BIG_SUPERBLOCKS * sb - 1234, sb, 11)
                elif g == "A" and f == PAGE:
                    self.arrays[g][f] = np.zeros(0, dtype=np.uint8)
                elif f in SLOTS[g]["large"]:
                    self.arrays[g][f] = self._fresh(g, f, (17 + f) * sb + 256 * T + 37 * T + 5, 100 + f)
                else:
                    self.arrays[g][f] = self._fresh(g, f, small[f - SLOTS[g]["small"][0]], 200 + f)

    def copy(self):
        m = Model.__new__(Model)
        m.arrays = {g: list(a) for g, a in self.arrays.items()}  # (arrays are never modified in place)
        m.turn, m.small_turn = self.turn, self.small_turn
        return m

    def _fresh(self, g, f, nbytes, seed):
        T = GROUPS[g][0]
        if f in NOISE[g]:
            return _data("rand", T, nbytes, seed)
        return _mixed_data(T, nbytes, _sb(T), seed) if f % 2 == 0 else _data("walk", T, nbytes, seed)

    def frames(self, g):
        return list(range(GROUPS[g][1]))

    def _next(self):
        self.turn += 1
        return self.turn

    def apply(self, step):
        op = getattr(self, "_" + step.cls)(step, np.random.default_rng([SEED, 3, step.i]))
        op.setdefault("error", None)
        op.setdefault("after", {})
        if op["error"] is None:
            for f, a in op["after"].items():
                self.arrays[step.group][f] = a
        return op

    # --- the classes
    def _new_array(self, step):
        g, f = step.group, step.frame
        T = GROUPS[g][0]
        sb = _sb(T)
        k = self._next()
        if step.regime == "large":
            n = (16 + k % 9) * sb + (k % 5) * 256 * T + 37 * T + 131 + k
        else:
            n = (127, 128, sb - 1, sb + 1, 100, sb, sb + 256 * T + 37, 5000)[self.small_turn % 8]
            self.small_turn += 1
        return self._fresh(g, f, n, 1000 + step.i)

    def _compress(self, step, rng):
        return {"before": {step.frame: self.arrays[step.group][step.frame]}, "after": {step.frame: self._new_array(step)}}

    _compress_async = _compress

    def _batch(self, step, rng):
        g = step.group
        after = {PAGE: np.zeros(0, dtype=np.uint8)} if g == "A" else {}
        return {"before": dict(enumerate(self.arrays[g])), "after": after}

    def _decompress(self, step, rng):
        return {"before": {step.frame: self.arrays[step.group][step.frame]}}

    def _ranges(self, step, rng):
        arr = self.arrays[step.group][step.frame]
        T = GROUPS[step.group][0]
        ranges = range_set(arr.size, _sb(T), 256 * T, rng, 1000 if step.regime == "large" else 4)
        return {"before": {step.frame: arr}, "ranges": ranges, "expect": [arr[lo:lo + n] for lo, n in ranges]}

    def _row_pick(self, rng, nrows, regime, unique):
        if nrows == 0:
            return []
        if unique:
            return [int(r) for r in rng.permutation(nrows)[:2000 if regime == "large" else 5]]
        rows = [int(r) for r in rng.integers(0, nrows, 3000 if regime == "large" else 4)]
        return rows + [0, nrows - 1, rows[0], rows[0]]

    def _gather(self, step, rng):
        arr = self.arrays[step.group][step.frame]
        rb = 300 if step.regime == "large" else 7
        rows = self._row_pick(rng, arr.size // rb, step.regime, False)
        return {"before": {step.frame: arr}, "row_bytes": rb, "rows": rows, "expect": _rows_of(arr, rows, rb)}

    def _pair_pick(self, rng, arrays, rb, regime, unique):
        counts = [a.size // rb for a in arrays]
        base = np.cumsum([0] + counts)
        total = int(base[-1])
        want = (3000 if unique else 4000) if regime == "large" else 8
        flat = rng.permutation(total)[:want] if unique else rng.integers(0, total, want)
        fids = np.searchsorted(base, flat, side="right") - 1
        return [int(f) for f in fids], [int(x - base[f]) for x, f in zip(flat, fids)]

    def _gather_batch(self, step, rng):
        g = step.group
        listed = self.frames(g) + ([1] if step.form != "own" else [])  # (the same frame twice, where the index is not the group's own)
        arrays = [self.arrays[g][f] for f in listed]
        rb = 300 if step.regime == "large" else 7
        fids, rows = self._pair_pick(rng, arrays, rb, step.regime, False)
        for k in ((PAGE - 1, len(listed) - 1) if g == "A" else (0, len(listed) - 1)):  # the neighbours of the page; the frame listed twice
            if arrays[k].size >= rb:
                fids += [k, k]
                rows += [arrays[k].size // rb - 1, 0]
        fids, rows = fids + fids[:2], rows + rows[:2]
        expect = np.stack([arrays[f][r * rb:(r + 1) * rb] for f, r in zip(fids, rows)])
        return {"before": dict(enumerate(self.arrays[g])), "listed": listed, "row_bytes": rb, "fids": fids, "rows": rows, "expect": expect}

    def _update(self, step, rng):
        arr = self.arrays[step.group][step.frame]
        rb = 512 if step.regime == "large" else 16
        rows = self._row_pick(rng, arr.size // rb, step.regime, True)
        src = rng.integers(0, 256, (len(rows), rb), dtype=np.uint8)
        return {"before": {step.frame: arr}, "after": {step.frame: _overlay(arr, rows, rb, src)}, "row_bytes": rb, "rows": rows, "src_rows": src}

    def _update_batch(self, step, rng):
        g = step.group
        arrays = self.arrays[g]
        rb = 512 if step.regime == "large" else 16
        fids, rows = self._pair_pick(rng, arrays, rb, step.regime, True)
        src = rng.integers(0, 256, (len(rows), rb), dtype=np.uint8)
        after = {}
        for f in sorted(set(fids)):
            mine = [k for k, x in enumerate(fids) if x == f]
            after[f] = _overlay(arrays[f], [rows[k] for k in mine], rb, src[mine])
        return {"before": dict(enumerate(arrays)), "after": after, "listed": self.frames(g), "row_bytes": rb, "fids": fids, "rows": rows, "src_rows": src}

    def _append_bytes(self, g, f, regime, rng, k):
        T = GROUPS[g][0]
        sb = _sb(T)
        have = self.arrays[g][f].size
        if regime == "large":
            n = (2 + k % 2) * sb + 1000 + 37 * T + k if have < 40 * sb else sb + 333
        else:
            n = (1, sb - have % sb, 77)[k % 3] if have < 3 * sb or (g == "A" and f == BIG) else (1, 77)[k % 2]
        return _data(("rand", "walk")[k % 2], T, n, 2000 + k)

    def _append(self, step, rng):
        g, f = step.group, step.frame
        src = self._append_bytes(g, f, step.regime, rng, self._next())
        return {"before": {f: self.arrays[g][f]}, "after": {f: np.concatenate([self.arrays[g][f], src])}, "src": src}

    def _append_batch(self, step, rng):
        g = step.group
        k = self._next()
        srcs, after = {}, {}
        for f in self.frames(g):
            if g == "A" and f == PAGE:
                T = GROUPS[g][0]
                n = 0 if self.arrays[g][f].size else (_sb(T) + 5 if step.regime == "large" else (127, 300)[k % 2])
                src = _data("walk", T, n, 3000 + k) if n else np.zeros(0, dtype=np.uint8)
            elif (f + k) % 3 == 0:
                src = np.zeros(0, dtype=np.uint8)
            else:
                src = self._append_bytes(g, f, step.regime, rng, k + f)
            srcs[f] = src
            if src.size:
                after[f] = np.concatenate([self.arrays[g][f], src])
        return {"before": dict(enumerate(self.arrays[g])), "after": after, "listed": self.frames(g), "srcs": srcs}

    def _index(self, step, rng):
        return {"before": dict(enumerate(self.arrays[step.group])), "listed": self.frames(step.group)}

    def _host(self, step, rng):
        T = GROUPS[step.group][0]
        return {"before": {}, "host_array": _mixed_data(T, _sb(T) + 3000 + step.i, _sb(T), step.i), "level2_array": _data("walk", T, 3000 + step.i, step.i)}

    def _fail(self, step, rng):
        g, kind = step.group, step.kind
        T = GROUPS[g][0]
        sb = _sb(T)
        arrays = self.arrays[g]
        f = SLOTS[g]["large"][-1]
        if "damaged" in kind and kind != "gather_damaged":  # a partial last superblock that the device decodes
            f = next((x for x in SLOTS[g]["large"][::-1] + SLOTS[g]["small"] if arrays[x].size % sb >= 128), None)
            if f is None:
                raise ValueError("no frame with a partial last superblock of 128 bytes or more")
        arr = arrays[f]
        op = {"before": dict(enumerate(arrays)), "frame": f, "listed": self.frames(g)}
        if kind in ("gather_bad_row", "gather_damaged"):
            rows = [0, 1, arr.size // 100, 2] if kind == "gather_bad_row" else [0, 1, 2, 1]
            op.update(row_bytes=100, rows=rows, bad_slot=2 if kind == "gather_bad_row" else None, error=INVALID_PARAMETER if kind == "gather_bad_row" else INVALID_INPUT)
        elif kind == "gather_batch_bad_pair":
            op.update(row_bytes=100, fids=[0, f, len(arrays), f], rows=[0, 1, 0, 2], bad_slot=2, error=INVALID_PARAMETER)
        elif kind == "update_bad_row":
            op.update(row_bytes=64, rows=[1, arr.size // 64, 3], src_rows=rng.integers(0, 256, (3, 64), dtype=np.uint8), error=INVALID_PARAMETER)
        elif kind == "update_batch_bad_pair":
            op.update(row_bytes=64, fids=[0, len(arrays), f], rows=[1, 0, 3], src_rows=rng.integers(0, 256, (3, 64), dtype=np.uint8), error=INVALID_PARAMETER)
        elif kind == "update_dst_overflow":
            src = rng.integers(0, 256, (2, 64), dtype=np.uint8)
            op.update(row_bytes=64, rows=[1, 5], src_rows=src, would_be=_overlay(arr, [1, 5], 64, src), error=DST_OVERFLOW)
        elif kind == "append_dst_overflow":
            src = _data("rand", T, 500, step.i)
            op.update(src=src, would_be=np.concatenate([arr, src]), error=DST_OVERFLOW)
        elif kind == "append_damaged":
            op.update(src=_data("walk", T, 300, step.i), cut=10, error=SRC_OVERFLOW)
        elif kind == "append_batch_damaged":
            srcs = {x: (_data("walk", T, 100, step.i + x) if arrays[x].size else np.zeros(0, dtype=np.uint8)) for x in self.frames(g)}
            op.update(srcs=srcs, cut=10, error=SRC_OVERFLOW)
        else:
            raise ValueError(kind)
        return op
