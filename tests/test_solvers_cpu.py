"""CPU tests of the order-3 multistep solvers and the other options of the reference's ``UniPC.sample`` / ``DPM_Solver.sample``
(ns2vc_amd/schedule.py: build_table, run_table_numpy) against the reference's own loops (tests/golden/golden_v5.npz, make_golden_v5.py)."""
import hashlib
import os

import numpy as np
import pytest

from ns2vc_amd import schedule as S
from util import synthetic_x0

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "golden_v5.npz")
SKIPS = ("logSNR", "time_uniform", "time_quadratic")
# the g14 grid of make_golden_v5.py: (solver, steps, order, skip_type, lower_order_final, extra options)
SYN_CASES = [(s, n, o, k, lof, {}) for s in ("unipc", "dpmsolver++") for o in (1, 2, 3) for k in SKIPS for n in (3, 5, 8, 10, 20)
             for lof in (True, False) if n >= o and not (o == 1 and not lof)]
SYN_CASES += [("unipc", 10, 3, "logSNR", True, {"variant": "bh1"}), ("unipc", 8, 2, "time_uniform", True, {"variant": "bh1"}),
              ("dpmsolver++", 10, 2, "time_uniform", True, {"solver_type": "taylor"}),
              ("unipc", 10, 3, "time_uniform", True, {"denoise_to_zero": True}),
              ("dpmsolver++", 10, 3, "logSNR", True, {"denoise_to_zero": True}),
              ("unipc", 10, 3, "time_uniform", True, {"t_start": 0.8, "t_end": 0.01}),
              ("dpmsolver++", 10, 3, "logSNR", True, {"t_start": 0.9, "t_end": 0.005})]
# the prototype of these coefficients reached <= 2.2e-6 against the reference's float32 loops; measured <= 3.8e-6 over g14 (float32 host loop)
SYN_TOL = 5e-6
# sha256 prefixes of tables built by the parent commit's build_table (default options): they must not change by a bit
PARENT_HASHES = {("unipc", 20, 2): "6cb77e12246672c2", ("unipc", 5, 2): "534dd3437d45e33c", ("unipc", 10, 1): "6ddce0054b1328a5",
                 ("dpmsolver++", 20, 2): "587d2754ff567e7e", ("dpmsolver++", 9, 2): "5be6c9b0af4403ca", ("dpmsolver++", 3, 1): "e7d700203e162a83"}
PARENT_HASHES_DISCRETE = {("ddim", 30, 0.0): "91932967326039ab", ("ddim", 100, 1.0): "21b2dc77479a9b1a", ("ddpm", 1000, 0.0): "c55bb60b04862a44"}


def case_tag(solver, steps, order, skip, lof, extra):
    t = f"{'unipc' if solver == 'unipc' else 'dpmpp'}{order}_{skip}_{steps}" + ("" if lof else "_nolof")
    for k in sorted(extra):
        v = extra[k]
        t += f"_{k}" if v is True else f"_{k}{v}".replace(".", "p")
    return t


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def table_of(case):
    solver, steps, order, skip, lof, extra = case
    return S.build_table(solver, steps, order=order, skip_type=skip, lower_order_final=lof, **extra)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


# ---- build_table's surface -------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["unipc", "dpmsolver++"])
@pytest.mark.parametrize("skip", SKIPS)
def test_order3_and_every_option_accepted(solver, skip):
    t = S.build_table(solver, 10, order=3, skip_type=skip)
    assert t.coef.shape == (10, S.NCOEF) and np.isfinite(t.coef).all()
    assert S.has_history2(t)
    assert list(t.detail["order"][1:]) == ([1, 2, 3, 3, 3, 3, 3, 3, 2, 1] if solver == "unipc" else [1, 2] + [3] * 8)
    kw = {"variant": "bh1"} if solver == "unipc" else {"solver_type": "taylor"}
    t2 = S.build_table(solver, 8, order=3, skip_type=skip, lower_order_final=False, denoise_to_zero=True, t_start=0.9, t_end=0.01,
                       method="multistep", **kw)
    assert t2.steps == 9 and t2.coef.shape == (9, S.NCOEF)       # denoise_to_zero: one more row
    last = t2.coef[-1]
    assert (last[5], last[6]) == (0.0, -1.0) and not last[[3, 4, 7, 8, 9, 10, 11]].any()


@pytest.mark.parametrize("kw,match", [
    ({"solver": "unipc", "order": 3, "method": "singlestep"}, "multistep"),
    ({"solver": "dpmsolver++", "order": 2, "method": "singlestep_fixed"}, "multistep"),
    ({"solver": "dpmsolver++", "order": 3, "method": "adaptive"}, "multistep"),
    ({"solver": "unipc", "order": 3, "variant": "vary_coeff"}, "variant"),
    ({"solver": "dpmsolver++", "order": 2, "variant": "bh1"}, "variant"),
    ({"solver": "unipc", "order": 2, "solver_type": "taylor"}, "solver_type"),
    ({"solver": "unipc", "order": 4}, "order"),
    ({"solver": "dpmsolver++", "order": 5}, "order"),
    ({"solver": "unipc", "order": 3, "steps": 2}, "steps"),
    ({"solver": "unipc", "order": 3, "skip_type": "logsnr"}, "skip_type"),
    ({"solver": "unipc", "order": 3, "t_start": 0.5, "t_end": 0.6}, "t_end"),
])
def test_out_of_scope_inputs_rejected(kw, match):
    kw = dict(kw)
    solver, steps = kw.pop("solver"), kw.pop("steps", 10)
    with pytest.raises(ValueError, match=match):
        S.build_table(solver, steps, **kw)


@pytest.mark.parametrize("solver,steps,opt", [("ddim", 30, {"skip_type": "logSNR"}), ("ddim", 30, {"denoise_to_zero": True}),
                                              ("ddpm", 1000, {"lower_order_final": False}), ("ddpm", 1000, {"t_end": 0.01}),
                                              ("ddim", 30, {"variant": "bh1"})])
def test_discrete_solvers_take_no_options(solver, steps, opt):
    with pytest.raises(ValueError, match="options"):
        S.build_table(solver, steps, S.linear_betas(1000, np.float64), **opt)


def test_table_options_key():
    assert S.table_options({}) == () == S.table_options({"skip_type": "time_uniform", "t_end": None})
    assert S.table_options({"skip_type": "logSNR"}) == (("skip_type", "logSNR"),)
    with pytest.raises(TypeError, match="unknown"):
        S.table_options({"skiptype": "logSNR"})


# ---- existing tables do not move -------------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(PARENT_HASHES), ids=lambda k: f"{k[0]}{k[2]}-{k[1]}")
def test_default_tables_byte_identical_to_parent(key):
    solver, steps, order = key
    t = S.build_table(solver, steps, order=order)
    assert hashlib.sha256(t.coef.tobytes()).hexdigest()[:16] == PARENT_HASHES[key]
    explicit = S.build_table(solver, steps, None, order, 0.0, skip_type="time_uniform", lower_order_final=True, denoise_to_zero=False,
                             variant="bh2", solver_type="dpmsolver", t_start=None, t_end=None, method="multistep")
    assert explicit.coef.tobytes() == t.coef.tobytes()


@pytest.mark.parametrize("key", sorted(PARENT_HASHES_DISCRETE), ids=lambda k: f"{k[0]}{k[1]}-eta{k[2]}")
def test_discrete_tables_byte_identical_to_parent(key):
    solver, steps, eta = key
    t = S.build_table(solver, steps, S.linear_betas(1000, np.float64), eta=eta)
    assert hashlib.sha256(t.coef.tobytes()).hexdigest()[:16] == PARENT_HASHES_DISCRETE[key]


def test_history2_columns_zero_below_order3():
    for solver in ("unipc", "dpmsolver++"):
        for order in (1, 2):
            for steps in (order, 5, 10, 20, 50):
                for skip in SKIPS:
                    for lof in (True, False):
                        t = S.build_table(solver, steps, order=order, skip_type=skip, lower_order_final=lof)
                        assert not t.coef[:, 10:12].any() and not S.has_history2(t)
    b = S.linear_betas(1000, np.float64)
    for t in (S.build_table("ddim", 50, b, eta=1.0), S.build_table("ddpm", 1000, b)):
        assert not t.coef[:, 10:12].any()


def test_order3_rows_below_order3_keep_order2_coefficients():
    """warm-up and lower-order-final rows of an order-3 table are the order-2 table's rows (same grid): columns 0-9 equal"""
    for solver in ("unipc", "dpmsolver++"):
        t3, t2 = S.build_table(solver, 8, order=3), S.build_table(solver, 8, order=2)
        o3 = t3.detail["order"]
        for i in range(8):
            # row i computes update i+1 and corrects update i
            if o3[i + 1] <= 2 and (i == 0 or o3[i] <= 2):
                np.testing.assert_array_equal(t3.coef[i], t2.coef[i], err_msg=f"{solver} row {i}")


def test_logsnr_grid_is_uniform_in_lambda():
    sched = S.VPSchedule(S.linear_betas())
    t = S.build_table("unipc", 12, order=3, skip_type="logSNR")
    lam = np.array([sched.lam(x) for x in t.timesteps])
    d = np.diff(lam)
    assert np.abs(d / d.mean() - 1).max() < 1e-3
    # inverse_lambda (float64) inverts lam on the grid to float32 rounding of the grid
    np.testing.assert_allclose(sched.inverse_lambda(lam), t.timesteps, rtol=1e-5)


# ---- the host executor against the reference's own loops (g14) -------------------------------------
@pytest.mark.parametrize("case", SYN_CASES, ids=[case_tag(*c) for c in SYN_CASES])
def test_run_table_numpy_against_reference(case, gold):
    tag = case_tag(*case)
    x_T = gold["g14.x_T"]
    ref, times = gold[f"g14.{tag}.y"], gold[f"g14.{tag}.times"]
    t = table_of(case)
    assert t.steps == len(times)
    # model times: the table's t_model against the reference's model inputs, float32 either way (1e-6 relative; t = 0 exactly)
    np.testing.assert_allclose(t.t_model, times, rtol=1e-6, atol=2e-4)
    y = S.run_table_numpy(t, synthetic_x0, x_T)
    assert rel_l2(y, ref) <= SYN_TOL, rel_l2(y, ref)


def test_history2_executor_needed_for_order3(gold):
    """dropping the m_prev2 terms (columns 10-11) of an order-3 table moves the result far outside the bar: the columns carry the order"""
    case = ("unipc", 10, 3, "logSNR", True, {})
    t = table_of(case)
    t.coef[:, 10:12] = 0
    y = S.run_table_numpy(t, synthetic_x0, gold["g14.x_T"])
    assert rel_l2(y, gold[f"g14.{case_tag(*case)}.y"]) > 20 * SYN_TOL


def test_g15_tables_time_lists(gold):
    """the full-UNet cases of golden v5 evaluate at the times the tables hold"""
    cases = [("unipc", 10, 3, "logSNR", True, {}), ("unipc", 20, 3, "time_uniform", True, {}), ("dpmsolver++", 20, 3, "time_uniform", True, {}),
             ("unipc", 15, 3, "time_quadratic", True, {"variant": "bh1", "denoise_to_zero": True})]
    for c in cases:
        np.testing.assert_allclose(table_of(c).t_model, gold[f"g15.{case_tag(*c)}.times"], rtol=1e-6, atol=2e-4)
