"""The sequence and the model of tests/context_history.py, checked where they can be: without a GPU.  These are conditions on the
inputs of tests/test_gpu_context_history.py, not measurements: a seed that does not meet them is changed, the condition is not."""
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import context_history as ch
from test_gpu_ranges import _sb


@lru_cache(maxsize=None)
def _steps():
    return tuple(ch.steps_of(ch.sequence()))


@lru_cache(maxsize=None)
def _replayed():
    """[(step, op, sizes before, sizes after)] of the whole sequence on the model alone"""
    model = ch.Model()
    out = []
    for step in _steps():
        before = {g: list(a) for g, a in model.arrays.items()}
        op = model.apply(step)
        out.append((step, op, before, {g: list(a) for g, a in model.arrays.items()}))
    return out


def test_every_ordered_pair_of_classes_occurs_once():
    steps = _steps()
    assert len(steps) == 197 and len(ch.CLASSES) == 14
    pairs = Counter((s.prev, s.cls) for s in steps[1:])
    assert len(pairs) == 196 and set(pairs.values()) == {1}
    assert set(pairs) == {(a, b) for a in ch.CLASSES for b in ch.CLASSES}
    assert [s.i for s in steps] == list(range(197)) and {s.stream for s in steps} == {0, 1, 2}
    # the list alone gives the steps: a prefix replays the same calls
    specs = ch.sequence()
    assert ch.steps_of(specs[:50]) == list(steps[:50])


def test_small_calls_follow_large_ones_in_every_class():
    """every class at least three times in the small regime directly behind a large-regime step (all classes share the index
    workspace); the classes with tables of their own -- gather and update in both forms, append in both forms -- at least once
    behind a large-regime step of their own family; every class in every group"""
    steps = _steps()
    after_large = Counter(s.cls for p, s in zip(steps, steps[1:]) if s.regime == "small" and p.regime == "large")
    for c in ch.CLASSES:
        assert after_large[c] >= 3, (c, after_large[c])
        assert {s.group for s in steps if s.cls == c} == set(ch.GROUPS), c
    tables = (("gather", "gather_batch", "update", "update_batch"), ("append", "append_batch"))
    for family in tables:
        for c in family:
            assert any(s.cls == c and s.regime == "small" and p.regime == "large" and p.cls in family for p, s in zip(steps, steps[1:])), c


def test_every_index_form_in_every_class_that_takes_one():
    steps = _steps()
    for c in ch.SINGLE_INDEX + ch.MANY_INDEX:
        forms = Counter(s.form for s in steps if s.cls == c)
        assert all(forms[f] >= 3 for f in ("null", "own", "copy")), (c, forms)
    assert all(s.form is None for s in steps if s.cls not in ch.SINGLE_INDEX + ch.MANY_INDEX)
    # "own" only where the step before leaves an index the header calls valid, for the very frames of this step
    leaves_single = ("compress", "compress_async", "update", "append")
    leaves_many = ("index", "update_batch", "append_batch")
    for p, s in zip(steps, steps[1:]):
        if s.form != "own":
            continue
        if s.cls in ch.SINGLE_INDEX:
            assert (p.group, p.frame) == (s.group, s.frame), s
            assert p.cls in leaves_single or (p.cls in ("ranges", "gather") and p.form == "own"), s
        else:
            assert p.group == s.group, s
            assert p.cls in leaves_many or (p.cls == "gather_batch" and p.form == "own"), s


def test_every_failing_call_occurs():
    """all nine occur; (fail, X) occurs once for every X, so six `fail` steps are followed by a call of the family of what failed:
    each such pair holds an entry of that family, two different ones per family, and that call succeeds"""
    steps = _steps()
    assert {s.kind for s in steps if s.cls == "fail"} == set(ch.FAILS)
    followed = {}
    for p, s in zip(steps, steps[1:]):
        if p.cls == "fail" and s.cls in ch.FOLLOWED_BY:
            family = next(k for k, v in ch.FAMILIES.items() if s.cls in v)
            assert ch.FAIL_FAMILY[p.kind] == family, (p, s)
            followed.setdefault(family, set()).add(p.kind)
    assert all(len(followed[k]) == 2 for k in ch.FAMILIES), followed
    assert all(op["error"] is None for step, op, _, _ in _replayed() if step.cls != "fail")


def test_the_long_chain_and_the_empty_array_take_part():
    sb = _sb(4)
    big, page = set(), set()
    for step, op, before, after in _replayed():
        if step.group != "A" or step.cls not in ("gather_batch", "update_batch", "append_batch", "index"):
            continue
        assert before["A"][ch.BIG].size > 256 * sb
        if step.cls == "index" or (step.cls == "append_batch" and op["srcs"][ch.BIG].size) or ch.BIG in op.get("fids", ()):
            big.add(step.cls)
        if before["A"][ch.PAGE].size == 0:
            page.add(step.cls)
    assert big == page == {"gather_batch", "update_batch", "append_batch", "index"}, (big, page)
    # the page is started by append_batch and started anew by batch
    assert any(s.cls == "append_batch" and s.group == "A" and b["A"][ch.PAGE].size == 0 and a["A"][ch.PAGE].size for s, _, b, a in _replayed())
    assert any(s.cls == "append_batch" and ch.PAGE in op["srcs"] and op["srcs"][ch.PAGE].size == 0 and any(v.size == 0 for k, v in op["srcs"].items() if k != ch.PAGE)
               for s, op, _, _ in _replayed())


def test_the_model_is_consistent():
    for step, op, before, after in _replayed():
        g = step.group
        T = ch.GROUPS[g][0]
        sb = _sb(T)
        for other in ch.GROUPS:
            if other != g:
                assert all(x is y for x, y in zip(before[other], after[other])), step
        changed = {f for f in range(len(before[g])) if before[g][f] is not after[g][f]}
        assert changed == (set(op["after"]) if op["error"] is None else set()), step
        assert all(a.dtype == np.uint8 and a.ndim == 1 for a in after[g])
        for f, a in op["before"].items():
            assert a is before[g][f], step
        if step.cls == "fail":
            assert op["error"] in (ch.INVALID_PARAMETER, ch.SRC_OVERFLOW, ch.INVALID_INPUT, ch.DST_OVERFLOW) and not changed
            if "cut" in op:
                assert before[g][op["frame"]].size % sb >= 128
            continue
        if step.cls in ("compress", "compress_async"):
            n = after[g][step.frame].size
            assert (16 * sb <= n <= 25 * sb) if step.regime == "large" else (100 <= n <= sb + 256 * T + 37), (step, n)
            assert not (g == "A" and step.frame in (ch.BIG, ch.PAGE))
        elif step.cls == "ranges":
            arr = before[g][step.frame]
            assert len(op["expect"]) == len(op["ranges"])
            for (lo, n), e in zip(op["ranges"], op["expect"]):
                assert 0 <= lo and lo + n <= arr.size and np.array_equal(e, arr[lo:lo + n])
        elif step.cls == "gather":
            arr, rb = before[g][step.frame], op["row_bytes"]
            assert sb % rb and len(op["rows"]) > len(set(op["rows"])) and op["expect"].shape == (len(op["rows"]), rb)
            for r, e in zip(op["rows"], op["expect"]):
                assert (r + 1) * rb <= arr.size and np.array_equal(e, arr[r * rb:(r + 1) * rb])
        elif step.cls == "gather_batch":
            rb = op["row_bytes"]
            assert sb % rb and op["expect"].shape == (len(op["rows"]), rb)
            assert (len(op["listed"]) > len(set(op["listed"]))) == (step.form != "own")
            for f, r, e in zip(op["fids"], op["rows"], op["expect"]):
                arr = before[g][op["listed"][f]]
                assert (r + 1) * rb <= arr.size and np.array_equal(e, arr[r * rb:(r + 1) * rb])
        elif step.cls in ("update", "update_batch"):
            rb = op["row_bytes"]
            fids = op.get("fids", [step.frame] * len(op["rows"]))
            assert len(set(zip(fids, op["rows"]))) == len(op["rows"])
            want = {f: before[g][f].copy() for f in set(fids)}
            for f, r, s in zip(fids, op["rows"], op["src_rows"]):
                assert (r + 1) * rb <= want[f].size
                want[f][r * rb:(r + 1) * rb] = s
            assert set(want) == changed and all(np.array_equal(after[g][f], w) for f, w in want.items()), step
        elif step.cls == "append":
            assert np.array_equal(after[g][step.frame], np.concatenate([before[g][step.frame], op["src"]])) and op["src"].size
        elif step.cls == "append_batch":
            for f, s in op["srcs"].items():
                assert np.array_equal(after[g][f], np.concatenate([before[g][f], s]))
        elif step.cls == "batch":
            assert changed <= {ch.PAGE} and all(after["A"][ch.PAGE].size == 0 for _ in changed)
        else:
            assert not changed
        if step.regime == "large" and step.cls in ("gather", "update", "gather_batch", "update_batch"):
            assert len(op["rows"]) >= 2000
        if step.regime == "small" and step.cls in ("gather", "update", "gather_batch", "update_batch"):
            assert len(op["rows"]) <= 16


def test_small_sizes_and_appends_occur():
    """totals of sb - 1, sb + 1, 127 and 128; appends of one byte and of exactly what fills the last superblock"""
    totals, one, fill = set(), False, False
    for step, op, before, after in _replayed():
        T = ch.GROUPS[step.group][0]
        sb = _sb(T)
        if step.cls in ("compress", "compress_async") and step.regime == "small":
            n = after[step.group][step.frame].size
            totals.add({sb - 1: "sb-1", sb + 1: "sb+1"}.get(n, n))
        if step.cls == "append" or (step.cls == "append_batch" and step.regime == "small"):
            for f, s in (op["srcs"].items() if "srcs" in op else [(step.frame, op["src"])]):
                r = before[step.group][f].size % sb
                one |= s.size == 1
                fill |= s.size == sb - r and r > 0
    assert {"sb-1", "sb+1", 127, 128} <= totals and one and fill, (totals, one, fill)


@pytest.mark.parametrize("g", list(ch.GROUPS))
def test_every_group_has_noise_and_compressible_arrays(g):
    """noise: every byte value about equally often; the others far from it"""
    arrays = ch.Model().arrays[g]
    flat = lambda a: np.bincount(a[:1 << 16], minlength=256).max() / min(a.size, 1 << 16)  # noqa: E731
    assert all(flat(arrays[f]) < 0.03 for f in ch.NOISE[g] if arrays[f].size >= 4096)
    assert any(flat(a) > 0.03 for f, a in enumerate(arrays) if f not in ch.NOISE[g] and a.size)
