"""The solver-update and quantile kernels give the bits of the commit recorded in tests/golden/solver_bits_v2.json (tools/record_solver_bits.py ran
the cases of tests/solver_cases.py on that commit's library): every form, precision and branch of the family, by SHA-256 of every output array.
The other GPU tests pin the forms to each other; a change that shifted all of them by the same ulp would pass those and fails here."""
import json
import os

import pytest

import solver_cases

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "solver_bits_v2.json")


@pytest.fixture(scope="module")
def gold():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def lib():
    from ns2vc_amd import _lib
    return _lib.load()


def test_case_sets_agree(gold):
    assert sorted(gold["cases"]) == sorted(solver_cases.CASES), "the generator and the record disagree on the cases: record again ON THE PARENT"
    assert len(gold["parent_commit"]) == 40 and gold["hipcc"]


@pytest.mark.parametrize("case", solver_cases.CASES)
def test_bits_of_the_recorded_commit(case, gold, lib):
    want = gold["cases"][case]
    got = solver_cases.digest(solver_cases.run_case(lib, case))
    assert sorted(got) == sorted(want), (case, sorted(got), sorted(want))
    wrong = [k for k in sorted(want) if got[k] != want[k]]
    assert not wrong, f"case {case}: array(s) {', '.join(wrong)} differ from commit {gold['parent_commit'][:12]}"
