"""The slot loop -- ``Denoiser.open_slots``, ``SlotLoop.admit`` / ``admit_group`` / ``run`` / ``take`` / ``suspend`` / ``resume`` / ``close`` -- does
what the commit recorded in tests/golden/slot_calls_v1.json did (tools/record_slot_calls.py ran the cases of tests/slot_cases.py on that commit,
on the recording engine of tests/recording_engine.py): step by step the same engine calls with the same arguments in the same order, the same
exception type and text with no engine call made for a refusal, the same host state of every open loop afterwards (idle and finished slots, loop
step, pool rows in use, the five per-slot vectors) and the same fields of every ``Suspended`` that comes out.

One difference is allowed, in the steps named ``slot_cases.ADMISSION_FAILS`` ... -- an admission during which an engine call raises (case
``engine_raises``) or the precision self-check fails (case ``self_check[fails]``) -- and in their "vectors" alone: the recorded commit wrote an
admission's lengths, prompt lengths, seeds, scales and corrections into the loop's vectors first and left them there when the admission failed (a
failed resume already put them back); a failed admission now leaves the vectors as they were, which is what these steps assert instead.  The slots
stay idle either way, and the engine never reads an idle slot's entries.  Each of these steps is followed by the same admission succeeding, after
which the vectors agree again; everything else in these steps, and every other step, is held to the record."""
import json
import os

import pytest

import slot_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_calls_v1.json")
PARENT = "d09191c"


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_case_sets_agree(gold):
    assert sorted(gold["cases"]) == sorted(slot_cases.CASES), "the generator and the record disagree on the cases: record again ON THE PARENT"
    assert len(gold["parent_commit"]) == 40 and gold["parent_commit"].startswith(PARENT)
    refused = [s for c, steps in gold["cases"].items() if c.startswith("refusals") for s in steps if "error" in s]
    assert len(refused) > 80 and not any("calls" in s for s in refused)      # every recorded refusal came before any engine call


@pytest.mark.parametrize("case", slot_cases.CASES)
def test_steps_of_the_recorded_commit(case, gold, monkeypatch):
    want = gold["cases"][case]
    got = slot_cases.run_case(monkeypatch, case)      # (run_case(..., full=True) shows the arguments behind a differing hash)
    assert [s["step"] for s in got] == [s["step"] for s in want]
    exempt = 0
    for k, (g, w) in enumerate(zip(got, want)):
        where = f"{case} / {w['step']}"
        if w["step"].startswith(slot_cases.ADMISSION_FAILS):
            exempt += 1
            assert "error" in g and [s["vectors"] for s in g["state"]] == [s["vectors"] for s in got[k - 1]["state"]], where
            assert [s["vectors"] for s in w["state"]] != [s["vectors"] for s in g["state"]], where      # (the recorded commit's had changed)
            g, w = (dict(s, state=[{n: v for n, v in e.items() if n != "vectors"} for e in s["state"]]) for s in (g, w))
        assert g == w, where
    assert exempt == {"engine_raises": 6, "self_check[fails]": 1}.get(case, 0)
