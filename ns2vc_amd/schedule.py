"""Host-side solver tables for the captured sampling loop.

All DPM-Solver++ / UniPC coefficients are data-independent scalars (SURVEY
fact 9), so they are computed ONCE per (betas, solver, steps) on the host in
float64 and handed to the engine as a flat float32 table; the device loop
indexes the table by step and contains no host synchronisation.

Reference math restated here:
  schedule      sampler/dpm_solver.py:100-154 (discrete VP, piecewise-linear log alpha)
  time grid     sampler/dpm_solver.py:474,1159-1160 (time_uniform), model time :278
  DPM-Solver++  sampler/dpm_solver.py:547-580 (1st order), :796-831 (2M), loop :1171-1213
  UniPC-bh2     sampler/uni_pc.py:471-567 (update), loop :606-658

Unified recurrence executed by the engine after the i-th denoiser evaluation
(i = 0 .. steps-1), all tensors elementwise, scalars from row i of the table:

    eps   = (xe - alpha*x0) / sigma ;  m = (xe - sigma*eps) / alpha      # x_start wrapper round trip
    x     = xbar - g0*d1 - g1*(m - m_prev)                               # (corrected) state at t_i
    xbar' = A*x - Bc*m                                                   # first-order part towards t_{i+1}
    d1'   = d1c*(m_prev - m)                                             # scaled backward difference
    xe'   = xbar' - pc*d1'                                               # point where the next evaluation happens
    m_prev' = m

with xbar = xe = x_T, d1 = m_prev = 0 before the first evaluation.  After the
last evaluation ``xe'`` is the sample.  For DPM-Solver++(2M): g0 = previous pc,
g1 = 0.  For UniPC: g0 = alpha_t*B_h*rho_0, g1 = alpha_t*B_h*rho_1, pc = alpha*B_h/2.

The two discrete samplers of the reference (model.py: ``ddim_sample``, ``p_sample_loop`` / ``p_sample``) are first-order
rows of the same recurrence (g0 = g1 = d1c = pc = 0, so xe' = xbar' = A*xe - Bc*m), plus a Gaussian term:

    xbar' += noise * z        z = ns2vc_amd.noise.gauss(seed_b, i, ...)  (the engine draws it on the device)

  DDIM   A = c*sqrt(1/a)/sqrt(1/a - 1),  Bc = c/sqrt(1/a - 1) - sqrt(a_next),  noise = eta*sqrt((1 - a/a_next)(1 - a_next)/(1 - a)),
         c = sqrt(1 - a_next - noise^2), a = alphas_cumprod[time]; the final pair (0, -1) returns x_start (A = 0, Bc = -1)
  DDPM   A = posterior_mean_coef2[t], Bc = -posterior_mean_coef1[t], noise = exp(0.5*posterior_log_variance_clipped[t]) (0 at t = 0)

A row with noise == 0 adds nothing at all (not 0*z), so every noise-free table keeps its bits.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np

# column layout of the per-step coefficient table (float32, NCOEF per row)
COEF_COLUMNS = ("t_model", "alpha", "sigma", "g0", "g1", "A", "Bc", "d1c", "pc", "noise", "_pad1", "_pad2")
NCOEF = len(COEF_COLUMNS)
SOLVERS = ("dpmsolver++", "unipc", "ddim", "ddpm")
DISCRETE_SOLVERS = ("ddim", "ddpm")      # tables over the integer timesteps of the model's own buffers; `order` does not apply


def linear_betas(n: int = 1000, dtype=np.float32) -> np.ndarray:
    """reference model.py:426-433: linspace in float64, stored as a float32 buffer (:471-473).  ``dtype=np.float64``: the
    betas the reference derives its other buffers from (alphas_cumprod, the posterior coefficients) before storing them."""
    scale = 1000.0 / n
    return np.linspace(scale * 1e-4, scale * 0.02, n, dtype=np.float64).astype(dtype)


class VPSchedule:
    """Discrete VP schedule in float64 (from the float32 betas the reference stores)."""

    def __init__(self, betas: np.ndarray):
        b32 = np.asarray(betas, dtype=np.float32)
        # the reference evaluates log(1-beta).cumsum() in float32; keep that so the
        # knots agree to float32 rounding, then continue in float64
        self.log_alpha = (0.5 * np.cumsum(np.log((1.0 - b32).astype(np.float32)).astype(np.float32), dtype=np.float32)).astype(np.float64)
        self.N = int(self.log_alpha.shape[0])
        self.knots = np.linspace(0.0, 1.0, self.N + 1, dtype=np.float32)[1:].astype(np.float64)

    def log_alpha_at(self, t: float) -> float:
        i = int(np.searchsorted(self.knots, t, side="left")) - 1
        i = min(max(i, 0), self.N - 2)
        x0, x1 = self.knots[i], self.knots[i + 1]
        y0, y1 = self.log_alpha[i], self.log_alpha[i + 1]
        return float(y0 + (t - x0) * (y1 - y0) / (x1 - x0))

    def alpha(self, t: float) -> float:
        return float(np.exp(self.log_alpha_at(t)))

    def sigma(self, t: float) -> float:
        return float(np.sqrt(1.0 - np.exp(2.0 * self.log_alpha_at(t))))

    def lam(self, t: float) -> float:
        la = self.log_alpha_at(t)
        return float(la - 0.5 * np.log(1.0 - np.exp(2.0 * la)))

    def timesteps(self, steps: int) -> np.ndarray:
        # the reference builds the grid with torch.linspace in float32
        return np.linspace(1.0, 1.0 / self.N, steps + 1, dtype=np.float32).astype(np.float64)

    def model_time(self, t: float) -> float:
        return float(np.float32((np.float32(t) - np.float32(1.0 / self.N)) * np.float32(self.N)))


@dataclass
class SolverTable:
    solver: str
    steps: int
    coef: np.ndarray          # (steps, NCOEF) float32
    timesteps: np.ndarray     # (steps+1,) continuous labels
    detail: Dict[str, np.ndarray]

    @property
    def t_model(self) -> np.ndarray:
        return self.coef[:, 0]


def build_table(solver: str, steps: int, betas: Optional[np.ndarray] = None, order: int = 2, eta: float = 0.0) -> SolverTable:
    """Coefficient table for ``steps`` denoiser evaluations (NFE == steps).

    ``ddim`` / ``ddpm`` need ``betas``, the model's own discrete schedule (pass the float64 betas, e.g.
    ``linear_betas(n, np.float64)``, to reproduce the reference's float32 buffers bit for bit); ``order`` does not apply to
    them.  ``eta`` is DDIM's noise scale (the reference's ``ddim_sampling_eta``); ``ddpm`` takes ``steps == len(betas)``."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if solver in DISCRETE_SOLVERS:
        return _discrete_table(solver, steps, betas, eta)
    if eta != 0.0:
        raise ValueError(f"eta applies to ddim only, not {solver!r}")
    if order not in (1, 2):
        raise ValueError("order must be 1 or 2")
    if steps < order:
        raise ValueError(f"steps ({steps}) must be >= order ({order})")   # dpm_solver.py:1172 / uni_pc.py:607
    sched = VPSchedule(linear_betas() if betas is None else betas)
    ts = sched.timesteps(steps)
    lam = np.array([sched.lam(t) for t in ts])
    alpha = np.array([sched.alpha(t) for t in ts])
    sigma = np.array([sched.sigma(t) for t in ts])
    coef = np.zeros((steps, NCOEF), dtype=np.float64)
    det = {k: np.zeros(steps + 1) for k in ("h", "rk", "B_h", "rho0", "rho1", "order")}

    def step_order(k: int) -> int:
        """order of the update that lands on ts[k], k = 1..steps"""
        if k < order:
            return k
        if solver == "unipc":
            return min(order, steps + 1 - k)                  # lower_order_final always, uni_pc.py:636-637
        return min(order, steps + 1 - k) if steps < 10 else order   # dpm_solver.py:1198-1201

    prev_pc = 0.0
    for i in range(steps):
        row = coef[i]
        row[0] = sched.model_time(ts[i])
        row[1], row[2] = alpha[i], sigma[i]
        # ---- correction of the state at t_i (uses the update that landed on ts[i])
        if i == 0:
            row[3] = row[4] = 0.0
        elif solver == "dpmsolver++":
            row[3], row[4] = prev_pc, 0.0
        else:
            k = i
            h = lam[k] - lam[k - 1]
            hh = -h
            h_phi_1 = np.expm1(hh)
            B_h = np.expm1(hh)
            ab = alpha[k] * B_h
            if step_order(k) == 1:
                rho0, rho1 = 0.0, 0.5                            # uni_pc.py:541-542
            else:
                rk = (lam[k - 2] - lam[k - 1]) / h
                h_phi_k = h_phi_1 / hh - 1.0
                b0 = h_phi_k / B_h
                b1 = (h_phi_k / hh - 0.5) * 2.0 / B_h
                rho0, rho1 = np.linalg.solve(np.array([[1.0, 1.0], [rk, 1.0]]), np.array([b0, b1]))   # :544
            row[3], row[4] = ab * rho0, ab * rho1
            det["rho0"][k], det["rho1"][k] = rho0, rho1
        # ---- move towards t_{i+1}
        k = i + 1
        h = lam[k] - lam[k - 1]
        phi = np.expm1(-h)                                       # = h_phi_1 = B_h (bh2) with hh = -h
        row[5] = sigma[k] / sigma[k - 1]
        row[6] = alpha[k] * phi
        det["h"][k], det["B_h"][k], det["order"][k] = h, phi, step_order(k)
        if step_order(k) == 2:
            rk = (lam[k - 2] - lam[k - 1]) / h                   # = -r0 of dpm_solver.py:822
            row[7] = 1.0 / rk
            row[8] = 0.5 * alpha[k] * phi
            det["rk"][k] = rk
        else:
            row[7] = row[8] = 0.0
        prev_pc = row[8]
    return SolverTable(solver, steps, coef.astype(np.float32), ts, det)


def _discrete_buffers(betas: np.ndarray) -> Dict[str, np.ndarray]:
    """the float32 buffers the reference registers (model.py NaturalSpeech2.__init__), computed in float64 as it does"""
    b = np.asarray(betas, dtype=np.float64)
    ac = np.cumprod(1.0 - b)
    ac_prev = np.concatenate([[1.0], ac[:-1]])
    pv = b * (1.0 - ac_prev) / (1.0 - ac)
    f = lambda v: np.asarray(v, dtype=np.float32)   # noqa: E731
    return {"alphas_cumprod": f(ac), "sqrt_recip_alphas_cumprod": f(np.sqrt(1.0 / ac)), "sqrt_recipm1_alphas_cumprod": f(np.sqrt(1.0 / ac - 1.0)),
            "posterior_log_variance_clipped": f(np.log(np.maximum(pv, 1e-20))),
            "posterior_mean_coef1": f(b * np.sqrt(ac_prev) / (1.0 - ac)), "posterior_mean_coef2": f((1.0 - ac_prev) * np.sqrt(1.0 - b) / (1.0 - ac))}


def ddim_times(steps: int, num_timesteps: int) -> List[int]:
    """model.py ddim_sample: torch.linspace(-1, T-1, steps+1) in float32, truncated, reversed -- the float32 grid truncates
    differently from a float64 one for 139 of the step counts 1..1000, so torch computes it"""
    import torch
    return list(reversed(torch.linspace(-1, num_timesteps - 1, steps=steps + 1).int().tolist()))


def _discrete_table(solver: str, steps: int, betas: Optional[np.ndarray], eta: float) -> SolverTable:
    if betas is None:
        raise ValueError(f"{solver} tables index the model's own discrete schedule: pass its betas (e.g. linear_betas(1000, np.float64))")
    bf = _discrete_buffers(betas)
    N = len(bf["alphas_cumprod"])
    if solver == "ddpm":
        if eta != 0.0:
            raise ValueError("eta applies to ddim only")
        if steps != N:
            raise ValueError(f"ddpm runs every timestep of the schedule: steps must be len(betas) = {N}, got {steps}")
        pairs = [(t, t - 1) for t in reversed(range(N))]
    else:
        if not 1 <= steps <= N:
            raise ValueError(f"ddim steps must be in [1, {N}], got {steps}")
        if eta < 0.0:
            raise ValueError(f"eta must be >= 0, got {eta}")
        times = ddim_times(steps, N)
        pairs = list(zip(times[:-1], times[1:]))
    d = np.float64
    coef = np.zeros((steps, NCOEF), dtype=np.float64)
    for i, (t, tn) in enumerate(pairs):
        row = coef[i]
        a = d(bf["alphas_cumprod"][t])
        row[0] = t
        row[1], row[2] = np.sqrt(a), np.sqrt(1.0 - a)     # the x_start round trip (any alpha, sigma != 0 reproduce x0 to rounding)
        if solver == "ddpm":
            row[5] = bf["posterior_mean_coef2"][t]
            row[6] = -d(bf["posterior_mean_coef1"][t])
            if t > 0:
                row[9] = np.exp(0.5 * d(bf["posterior_log_variance_clipped"][t]))
        elif tn < 0:
            row[5], row[6] = 0.0, -1.0                      # img = x_start
        else:
            # sigma and c in float32, as the reference evaluates them on its float32 buffers (1 - a/a_next cancels: float64 would
            # differ by ~1e-4 relative on 1000-step grids)
            f, a32, an32 = np.float32, bf["alphas_cumprod"][t], bf["alphas_cumprod"][tn]
            sig = f(eta) * np.sqrt((f(1) - a32 / an32) * (f(1) - an32) / (f(1) - a32))
            c = np.sqrt(np.maximum(f(1) - an32 - sig * sig, f(0)))
            r1, r2 = d(bf["sqrt_recip_alphas_cumprod"][t]), d(bf["sqrt_recipm1_alphas_cumprod"][t])
            # x_start*sqrt(a_next) + c*(r1*x - x_start)/r2 + sig*z   (predict_noise_from_start)
            row[5] = d(c) * r1 / r2
            row[6] = d(c) / r2 - d(np.sqrt(an32))
            row[9] = sig
    times_out = np.array([p[0] for p in pairs] + [pairs[-1][1]], dtype=np.float64)
    return SolverTable(solver, steps, coef.astype(np.float32), times_out, {"pairs": np.array(pairs, dtype=np.int64)})


def run_table_numpy(table: SolverTable, x0_fn: Callable[[np.ndarray, np.ndarray], np.ndarray], x_T: np.ndarray,
                    trace: Optional[List[np.ndarray]] = None, noise_fn: Optional[Callable[[int], np.ndarray]] = None) -> np.ndarray:
    """Host executor of the unified recurrence (float32), used by CPU tests to pin
    the tables against the oracle samplers.  ``x0_fn(x, t_model[B]) -> x0``.  ``noise_fn(i)`` -> the standard normals of
    step i, shaped like x_T (ns2vc_amd.noise.gauss), for tables with a nonzero noise column."""
    f = np.float32
    xbar = x_T.astype(f).copy()
    xe = xbar.copy()
    d1 = np.zeros_like(xbar)
    m_prev = np.zeros_like(xbar)
    B = x_T.shape[0]
    for i in range(table.steps):
        t_model, alpha, sigma, g0, g1, A, Bc, d1c, pc = (f(v) for v in table.coef[i, :9])
        x0 = x0_fn(xe, np.full((B,), t_model, dtype=f)).astype(f)
        eps = (xe - alpha * x0) / sigma
        m = (xe - sigma * eps) / alpha
        x = xbar - g0 * d1 - g1 * (m - m_prev)
        xbar = A * x - Bc * m
        if table.coef[i, 9] != 0:
            if noise_fn is None:
                raise ValueError(f"step {i} of this {table.solver} table adds noise: pass noise_fn")
            xbar = xbar + f(table.coef[i, 9]) * np.asarray(noise_fn(i), dtype=f)
        d1 = d1c * (m_prev - m)
        xe = xbar - pc * d1
        m_prev = m
        if trace is not None:
            trace.append(xe.copy())
    return xe
