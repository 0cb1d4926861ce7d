"""The case table of tests/split_edge_cases.py against the CPU oracle alone: every case is what its name says (pixels, lines, sub-lines at the deciding
threshold), the oracle finds or does not find the hand-derived threshold, the two sides of every arithmetic edge give different answers, and the table
as a whole reaches every initial action and every way a search can end.  No case is skipped or filtered: a failed precondition fails the test."""
import collections
import functools
import numpy as np
import pytest
from oracle import oracle
import split_edge_cases as sc


def detect_params(case):
    n, H, W = case.frames.shape
    return oracle.make_params(W, H, cm_per_pixel=case.cm, **case.detect_kw)


@functools.lru_cache(maxsize=None)
def answers(name):
    """-> [(Blob or None, blob record, lines, oracle SplitInfo or None)] of every detect blob of the case, in frame and table order"""
    case = sc.table()[name]
    sp = oracle.split_params(**case.oracle_split_kw())
    out = []
    for f, frame in enumerate(case.frames):
        blobs, runs, px = oracle.segment(frame, case.bg, detect_params(case))
        spec = {b.origin: b for b in case.blobs if b.frame == f} if case.blobs is not None else None
        if spec is not None:
            assert sorted(spec) == sorted((int(b["x0"]), int(b["y0"])) for b in blobs), "the frame's blobs are not the constructed ones"
        for b in blobs:
            s = spec[(int(b["x0"]), int(b["y0"]))] if spec is not None else None
            pn = s.presumed if s else case.presumed_all
            rs, ps = runs[b["run_begin"]:b["run_begin"] + b["n_runs"]], px[b["pix_begin"]:b["pix_begin"] + b["n_pixels"]]
            want = oracle.split_search(rs, ps, case.bg, case.method, sp, pn, case.connectivity) if pn > 0 else None
            out.append((s, b, (rs, ps), want))
    return out


def in_capacity(b):
    return b["n_pixels"] <= sc.S_PX_HUGE and b["n_runs"] <= sc.S_RUNS_HUGE


@pytest.mark.parametrize("name", sc.NAMES)
def test_case_is_what_it_says(name):
    case = sc.table()[name]
    sp = oracle.split_params(**case.oracle_split_kw())
    found = 0
    for s, b, (rs, ps), want in answers(name):
        if want is not None and want.threshold >= 0:
            found += 1
        if s is None:
            continue
        assert s.n_pixels is None or b["n_pixels"] == s.n_pixels
        assert s.n_runs is None or b["n_runs"] == s.n_runs
        if s.sublines is not None:
            lines = len(oracle.threshold_blob(rs, ps, case.bg, case.method, s.sub_at, case.connectivity)[1])
            assert lines == s.sublines
        if s.outcome == "skipped":
            assert s.presumed <= 0
            continue
        if s.outcome == "capacity":
            # beyond every size class, or more sub-lines than its class holds at a threshold the search reaches; the oracle itself has no capacity
            cap = sc.S_SUB_HUGE if b["n_pixels"] > sc.S_PX or b["n_runs"] > sc.S_RUNS else sc.S_SUB
            assert not in_capacity(b) or s.sublines > cap
            assert s.threshold == -1
            continue
        assert in_capacity(b)
        assert (want.threshold, want.effective_threshold) == (s.threshold, s.effective), (want.threshold, want.effective_threshold)
        if s.initial_action is not None:
            assert want.initial_action == s.initial_action
        if s.n_result is not None:
            assert want.n_result == s.n_result
        if s.min_max is not None:
            assert (want.min_pixel, want.max_pixel) == s.min_max
        begin = max(sp.initial_threshold, want.min_pixel)
        full = 1 + max(0, want.max_pixel - begin)            # the initial evaluation and every threshold of the complete search
        if s.outcome == "found":
            assert want.threshold >= 0 and want.initial_action != sc.KEEP_ABORT
        elif s.outcome == "initial":
            assert want.initial_action == sc.KEEP_ABORT and want.n_tried == 1 and want.threshold == sp.initial_threshold
        elif s.outcome in ("guard", "nosearch"):
            assert want.threshold == -1 and want.n_tried == 1 and want.max_pixel > begin
            assert (s.presumed == 1) == (s.outcome == "nosearch")
        elif s.outcome == "exhaust" and case.algorithm == 1:
            assert want.threshold == -1 and want.n_tried == full
        elif s.outcome == "abort":
            assert case.algorithm == 1 and want.threshold == -1 and 1 < want.n_tried < full
            t = begin + want.n_tried - 2                      # the last threshold tried is the one that was ABORTed
            left = int(oracle.threshold_blob(rs, ps, case.bg, case.method, t, case.connectivity)[0]["n_pixels"].sum())
            ms = np.float32(case.split_kw.get("blob_split_max_shrink", 0.2))
            assert np.float32(left) * sc.sqcm(case.cm) < ms * np.float32(want.first_size)
            more = int(oracle.threshold_blob(rs, ps, case.bg, case.method, t - 1, case.connectivity)[0]["n_pixels"].sum())
            assert not np.float32(more) * sc.sqcm(case.cm) < ms * np.float32(want.first_size)
        else:
            assert s.outcome == "exhaust" and want.threshold == -1
    assert found >= case.min_found


def answer_of(name):
    (s, b, _, want), = answers(name)
    return (want.threshold, want.effective_threshold, want.initial_action, want.n_result)


def test_edges_have_two_sides():
    """family c: within one edge, the cases on different sides get different answers from the oracle, those on one side the same"""
    groups = collections.defaultdict(list)
    for name in sc.NAMES:
        case = sc.table()[name]
        assert (case.edge is not None) == (case.family == "c")
        if case.edge:
            groups[case.edge[0]].append((case.edge[1], answer_of(name)))
    assert len(groups) >= 14
    for g, members in groups.items():
        sides = collections.defaultdict(set)
        for side, ans in members:
            sides[side].add(ans)
        assert len(sides) >= 2, g
        assert all(len(a) == 1 for a in sides.values()), (g, sides)
        assert len(set(next(iter(a)) for a in sides.values())) == len(sides), (g, sides)


def test_table_reaches_every_action_and_outcome():
    table = sc.table()
    assert {c.family for c in table.values()} == set("abcdef")
    actions, outcomes = set(), set()
    for name in sc.NAMES:
        for s, b, _, want in answers(name):
            if want is not None:
                actions.add(want.initial_action)
            if s is not None:
                outcomes.add(s.outcome)
    assert {sc.KEEP_ABORT, sc.REMOVE, sc.TOO_FEW} <= actions
    assert {"found", "initial", "abort", "exhaust", "guard", "nosearch", "capacity", "skipped"} <= outcomes


def test_cm_per_pixel_is_a_widened_float():
    """the library squares the double and rounds, the reference squares the float: equal for every cm_per_pixel of the table, and the table's three
    values are ones for which the plain double would not be"""
    for c in sc.table().values():
        assert np.float32(c.cm * c.cm) == sc.sqcm(c.cm)
        for a, b in c.ranges:
            assert a < b
    assert {c.cm for c in sc.table().values()} >= {sc.f32cm(v) for v in (0.37, 0.1, 0.0173)}
    for v in (0.37, 0.1, 0.0173):
        assert np.float32(v * v) != sc.sqcm(v)
