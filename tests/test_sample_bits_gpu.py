"""``Denoiser.sample`` / ``sample_long`` return the bits of the commit recorded in tests/golden/sample_bits_v1.json (tools/record_sample_bits.py ran
the call sequence of tests/sample_cases.py on that commit): the SHA-256 of every returned latent, and the step graphs the head and the tail engine
had captured after every call -- a setup order that recaptures more often shows there.  Equality is the condition: the launches are the same."""
import json
import os

import pytest

import sample_cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_bits_v1.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module", params=["fp16", "fp32"])
def bits(request):
    """one Denoiser per precision, the whole sequence once"""
    from ns2vc_amd.pipeline import Denoiser
    from ns2vc_amd.weights import procedural_state_dict
    return request.param, sample_cases.run_bits(Denoiser(procedural_state_dict(seed=0), precision=request.param))


def test_call_sets_agree(gold):
    assert len(gold["parent_commit"]) == 40 and sorted(gold["calls"]) == ["fp16", "fp32"]
    for prec in gold["calls"]:
        assert sorted(gold["calls"][prec]) == sorted(sample_cases.BIT_CALLS), "the sequence and the record disagree: record again ON THE PARENT"


@pytest.mark.parametrize("label", sample_cases.BIT_CALLS)
def test_bits_and_captures_of_the_recorded_commit(label, bits, gold):
    prec, got = bits
    want = gold["calls"][prec][label]
    print(f"{prec} {label}: {got[label]} (recorded {want})")
    assert got[label]["sha256"] == want["sha256"], f"{prec} {label}: the latent differs from commit {gold['parent_commit'][:12]}"
    assert (got[label]["head_captures"], got[label]["tail_captures"]) == (want["head_captures"], want["tail_captures"]), f"{prec} {label}: graph captures"
