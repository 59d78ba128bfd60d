"""``Denoiser.sample``, ``denoise``, ``sample_long``, ``sample_sharded`` and the slot loop send their engines what the commit recorded in
tests/golden/sample_calls_v1.json sent (tools/record_sample_calls.py ran the cases of tests/sample_cases.py on that commit, on the recording
engine of tests/recording_engine.py): per step the calls of the 16-bit head and of the fp32 tail with a hash of their arguments, the warnings, the
hash of the result, and for a refusal the exception's type and text with no engine call made.

One difference is allowed, so that one setup order serves both engines: in the tail's sequence ``load_sampler`` may stand behind
``set_guidance`` / ``set_x0_correction*``.  The tail is compared with its ``load_sampler`` entries taken out, and those separately: the same
entries, each in front of the ``set_condition`` of the step's loop on the tail."""
import json
import os

import pytest
import torch

import sample_cases

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_calls_v1.json")
PARENT = "9fdce08"


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


def test_case_sets_agree(gold):
    assert sorted(gold["cases"]) == sorted(sample_cases.CASES), "the generator and the record disagree on the cases: record again ON THE PARENT"
    assert len(gold["parent_commit"]) == 40 and gold["parent_commit"].startswith(PARENT)
    refused = [s for steps in gold["cases"].values() for s in steps if "error" in s]
    assert len(refused) > 100 and not any("head" in s or "tail" in s for s in refused)      # every recorded refusal came before any engine call


@pytest.mark.parametrize("case", sample_cases.CASES)
def test_calls_of_the_recorded_commit(case, gold, monkeypatch):
    want = gold["cases"][case]
    got = sample_cases.run_case(monkeypatch, case)      # (run_case(..., full=True) shows the arguments behind a differing hash)
    assert [s["step"] for s in got] == [s["step"] for s in want]
    for g, w in zip(got, want):
        where = f"{case} / {w['step']}"
        assert g.get("error") == w.get("error"), where
        if "error" in w:
            assert "head" not in g and "tail" not in g, where
            continue
        assert g.get("head", "").split() == w.get("head", "").split(), where
        gt, wt = g.get("tail", "").split(), w.get("tail", "").split()
        assert [c for c in gt if not c.startswith("load_sampler:")] == [c for c in wt if not c.startswith("load_sampler:")], where
        assert [c for c in gt if c.startswith("load_sampler:")] == [c for c in wt if c.startswith("load_sampler:")], where
        names = [c.split(":")[0] for c in gt]
        if "load_sampler" in names and "set_condition" in names:
            # (the loop's own condition is the step's last: a first call's self-check binds the tail once before, with no table loaded)
            assert max(i for i, n in enumerate(names) if n == "load_sampler") < max(i for i, n in enumerate(names) if n == "set_condition"), where
        assert g.get("warnings") == w.get("warnings"), where
        assert g.get("result") == w.get("result"), where


def test_the_guards_redo_starts_from_the_same_x_T_and_seeds(monkeypatch):
    """outside the record (its redo cases pass ``noise=``): the redo of the LayerNorm guard runs the same request again -- with ``noise=None`` and a
    ``generator=`` from the x_T and the seeds the first run drew, and the generator is not drawn from a second time.  (The recorded commit's redo
    restated the call by hand and left ``generator=`` out; it passed the drawn noise and seeds on, so it did the same.)  Two Denoisers, the guard
    firing on the first call of one only"""
    import recording_engine as R
    from ns2vc_amd.pipeline import Denoiser
    c, p, _ = sample_cases._inputs(2, 40)
    runs = []
    for ratio in (1.0, 100.0):
        rec = R.install(monkeypatch, R.Recording())
        rec.ln_ratio = ratio
        d = Denoiser({}, precision="fp32")
        g = torch.Generator().manual_seed(123)
        d.sample(c, p, solver="ddim", steps=5, eta=0.5, generator=g)
        runs.append(([a["x"] for a in rec.of("sample")], [a["seeds"] for a in rec.of("set_seeds")], g.get_state()))
    ref = torch.Generator().manual_seed(123)
    first = R.digest(torch.randn((2, 100, sample_cases.T), generator=ref))
    (x0, seeds0, state0), (x1, seeds1, state1) = runs
    assert x0 == [first] and x1 == [first, first]
    assert len(seeds0) == 1 and seeds1 == seeds0 * 2
    assert torch.equal(state0, state1)
