"""The three host loops of ``ns2vc_amd/schedule.py`` compute what the commit recorded in tests/golden/host_loops_v1.json computed
(tools/record_host_loops.py ran the cases of tests/host_loop_cases.py on that commit): per case the digests of the result, of every trace entry,
of what every ``x0_fn`` and ``noise_fn`` call was given, and for a refusal the exception's text.  And the loops hold no statement of the
recurrence of their own: with ``schedule.solver_update`` replaced by the identity every one of them returns its start state."""
import json
import os

import numpy as np
import pytest

import host_loop_cases as H
from ns2vc_amd import schedule as S

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "host_loops_v1.json")
PARENT = "0171cd9"


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_case_sets_agree(gold):
    assert list(gold["cases"]) == H.CASES, "the generator and the record disagree on the cases: record again ON THE PARENT"
    assert len(gold["parent_commit"]) == 40 and gold["parent_commit"].startswith(PARENT)
    refused = [c for c, r in gold["cases"].items() if "error" in r]
    assert refused == [c for c in H.CASES if c.startswith("refuse/")] and all(set(gold["cases"][c]) == {"error"} for c in refused)
    ran = [r for r in gold["cases"].values() if "error" not in r]
    assert all(len(r["trace"]) == len(r["x0_calls"]) for r in ran)
    assert sum(bool(r["noise_calls"]) for r in ran) >= 12 and any(len(r["trace"]) == 1000 for r in ran)


def test_inputs_are_what_the_record_was_taken_on():
    """the integer hash and the stand-in denoiser, pinned by value: exact in float32 on any machine"""
    a = H.hash_array(1, (4,))
    assert a.dtype == np.float32 and np.abs(H.hash_array(7, (1000,))).max() < 3.0 and len(np.unique(H.hash_array(7, (1000,)))) > 990
    assert np.array_equal(a, H.hash_array(1, (2, 2)).reshape(-1)) and not np.array_equal(a, H.hash_array(2, (4,)))
    y = H.stand_in(np.array([[[3.0, -1.0]]], np.float32), np.array([4.0], np.float32))
    f = np.float32
    assert np.array_equal(y, np.array([[[f(0.9) * f(3) / f(4) + f(0.05) * f(4) / f(5), f(0.9) * f(-1) / f(2) + f(0.05) * f(4) / f(5)]]], f))


@pytest.mark.parametrize("case", H.CASES)
def test_the_loops_of_the_recorded_commit(case, gold):
    want, got = gold["cases"][case], H.run_case(case)
    assert got.get("error") == want.get("error")
    for key in ("x0_calls", "noise_calls", "trace", "result"):      # (what the model was asked first: the first difference is the earliest)
        assert got.get(key) == want.get(key), f"{case}: {key}"


# ---- no second statement of the recurrence --------------------------------------------------------------------------------------------------
def _identity(c, hist2, x0, xe, xbar, d1, m_prev, m_prev2, correct=None, z=None):
    return xe, xbar, d1, m_prev, m_prev2


@pytest.mark.parametrize("name,how", [("unipc2", "plain"), ("unipc3_logsnr", "dyn"), ("dpmpp3", "clamp"), ("unipc2_dtz", "plain"),
                                      ("ddim_eta1", "plain")])
def test_run_table_numpy_has_no_update_of_its_own(name, how, monkeypatch):
    monkeypatch.setattr(S, "solver_update", _identity)
    x, trace, rec = H.x_T(1), [], H.Recorder(H.SHAPE)
    kw = dict(correct_x0=dict(H.DYN, lengths=H.LENGTHS) if how == "dyn" else dict(H.CLAMP)) if how != "plain" else {}
    y = S.run_table_numpy(H.tables()[name], rec.x0, x, trace, rec.noise, **kw)
    assert np.array_equal(y, x) and all(np.array_equal(t, x) for t in trace) and len(trace) == H.tables()[name].steps


@pytest.mark.parametrize("kw", [{}, dict(starts=H.STARTS), dict(scales=H.SCALES), dict(correct_x0=[dict(H.DYN, lengths=12), dict(H.CLAMP), None])],
                         ids=["right_aligned", "starts", "guided", "correct_list"])
def test_run_tables_numpy_has_no_update_of_its_own(kw, monkeypatch):
    monkeypatch.setattr(S, "solver_update", _identity)
    kw = dict(kw)
    tabs = H.item_tables(starts=kw.pop("starts", None))
    scales = kw.pop("scales", None)
    if scales is not None:
        kw["guided_x0"] = np.asarray(scales, np.float32)
    x, trace, rec = H.x_T(3), [], H.Recorder(H.SHAPE[1:], guided=scales is not None)
    y = S.run_tables_numpy(tabs, rec.x0, x, trace, rec.noise, **kw)
    assert np.array_equal(y, x) and all(np.array_equal(t, x) for t in trace) and len(trace) == tabs.steps


@pytest.mark.parametrize("make", [H.timeline, lambda: H.timeline("det"), lambda: H.timeline(own=[dict(H.DYN, lengths=7), dict(H.CLAMP), None]),
                                  lambda: H.timeline(hold=[H.slot_hold(), None, H.KEEP])], ids=["mixed", "det", "own", "held"])
def test_run_slots_numpy_has_no_update_of_its_own(make, monkeypatch):
    monkeypatch.setattr(S, "solver_update", _identity)
    tl, rec = make(), H.Recorder(H.SHAPE[1:])
    res = S.run_slots_numpy(tl, rec.x0, H.SHAPE, None, rec.noise)
    assert [len(r) for r in res] == [2, 0, 1]
    for items, out in zip(tl, res):
        for item, y in zip(items, out):
            assert np.array_equal(y, item[2])
