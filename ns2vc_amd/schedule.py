"""Host-side solver tables for the captured sampling loop.

All DPM-Solver++ / UniPC coefficients are data-independent scalars (SURVEY
fact 9), so they are computed ONCE per (betas, solver, steps) on the host in
float64 and handed to the engine as a flat float32 table; the device loop
indexes the table by step and contains no host synchronisation.

Reference math restated here:
  schedule      sampler/dpm_solver.py:100-154 (discrete VP, piecewise-linear log alpha)
  time grid     sampler/dpm_solver.py:474,1159-1160 (time_uniform), model time :278
  time grids    sampler/dpm_solver.py:453-479, sampler/uni_pc.py:305-320 (logSNR | time_uniform | time_quadratic)
  DPM-Solver++  sampler/dpm_solver.py:547-580 (1st order), :796-831 (2M), :854-904 (3M), loop :1171-1213
  UniPC-bh      sampler/uni_pc.py:471-588 (update), loop :606-658

Unified recurrence executed by the engine after the i-th denoiser evaluation
(i = 0 .. rows-1), all tensors elementwise, scalars from row i of the table:

    eps   = (xe - alpha*x0) / sigma ;  m = (xe - sigma*eps) / alpha      # x_start wrapper round trip
    x     = xbar - g0*d1 - g1*(m - m_prev)                               # (corrected) state at t_i
    xbar' = A*x - Bc*m                                                   # first-order part towards t_{i+1}
    d1'   = d1c*(m_prev - m) + d2c*(m_prev2 - m)                         # stored residual (backward differences)
    xe'   = xbar' - pc*d1' - pe*(m_prev2 - m)                            # point where the next evaluation happens
    m_prev2' = m_prev ;  m_prev' = m

with xbar = xe = x_T, d1 = m_prev = m_prev2 = 0 before the first evaluation.  After the
last evaluation ``xe'`` is the sample.  On the host ``solver_update`` is where this recurrence is stated (the twin of common.h ``solver_elem`` +
``solver_xe``); ``run_table_numpy``, ``run_tables_numpy`` and ``run_slots_numpy`` drive it and contain none of it.
Rows of order <= 2 have d2c = pe = 0 (columns 10-11): a table whose columns 10-11 are all zero runs without the m_prev2 history at all (the engine's update keeps its order-2 arithmetic).
Update k (landing on t_k, computed by row k-1, corrected by row k), h = lam_k - lam_{k-1},
rk_j = (lam_{k-1-j} - lam_{k-1}) / h:
  DPM-Solver++  g0 = previous pc, g1 = 0.  Order 2: d1c = 1/rk_1, pc = alpha_k*phi1/2 ('dpmsolver') or -alpha_k*(phi1/h + 1)
                ('taylor', dpm_solver.py:824-829).  Order 3 (3M, dpm_solver.py:854-904): alpha*phi2*D1 - alpha*phi3*D2 written as
                c_u*(m_prev - m) + c_v*(m_prev2 - m); pc = alpha_k*phi1/2, d1c = -c_u/pc, d2c = -c_v/pc, pe = 0, so xe' is the
                3M state and the next row's x = xbar - pc*d1 = xe.
  UniPC-bh      aB = alpha_k*B_h (B_h = expm1(-h) for bh2, -h for bh1, uni_pc.py:509-514).  Order 2: g0 = aB*rho_0,
                g1 = aB*rho_1, pc = aB/2, d1c = 1/rk_1.  Order 3: rc = the 3x3 ``rhos_c`` solve, rp = the 2x2 ``rhos_p`` solve
                (uni_pc.py:516-541); d1c = 1/rk_1, d2c = (rc_1/rc_0)/rk_2 (so rc_0*d1' is the corrector residual),
                pc = aB*rp_0, pe = aB*rp_1/rk_2 - pc*d2c; the correcting row has g0 = aB*rc_0, g1 = aB*rc_2.
``denoise_to_zero``: one more row at t_0 (A = 0, Bc = -1: xe' = x_start of that evaluation), so the table has steps + 1 rows.

The two discrete samplers of the reference (model.py: ``ddim_sample``, ``p_sample_loop`` / ``p_sample``) are first-order
rows of the same recurrence (g0 = g1 = d1c = pc = 0, so xe' = xbar' = A*xe - Bc*m), plus a Gaussian term:

    xbar' += noise * z        z = ns2vc_amd.noise.gauss(seed_b, i, ...)  (the engine draws it on the device)

  DDIM   A = c*sqrt(1/a)/sqrt(1/a - 1),  Bc = c/sqrt(1/a - 1) - sqrt(a_next),  noise = eta*sqrt((1 - a/a_next)(1 - a_next)/(1 - a)),
         c = sqrt(1 - a_next - noise^2), a = alphas_cumprod[time]; the final pair (0, -1) returns x_start (A = 0, Bc = -1)
  DDPM   A = posterior_mean_coef2[t], Bc = -posterior_mean_coef1[t], noise = exp(0.5*posterior_log_variance_clipped[t]) (0 at t = 0)

A row with noise == 0 adds nothing at all (not 0*z), so every noise-free table keeps its bits.

Known frames (``hold=`` of the two host loops, ``Engine.set_known``).  Per loop item b a frame mask K_b inside [0, L_b) -- L_b =
lengths[b] or T -- and a known latent k_b.  At every evaluation, before anything reads the x0 the model wrote:

    x0[b, c, t] = k_b[c, t]    for t in K_b, every latent channel c      (the engine's pad columns of such a row: 0; all other rows keep every bit)

Under guidance both halves are overwritten; ``guided_x0(k, k, s)`` is k at every scale, so the update does not change.  The start state of a
held frame is ``known_start``: x_T = alpha_0 k + sigma_0 noise in float32, alpha_0 and sigma_0 columns 1 and 2 of the item's first row.  The
recurrence is linear in x0 and m is constant there, so the backward differences vanish and a held frame follows the forward marginal with that
one noise at any order, for UniPC and DPM-Solver++ alike: x_i = alpha_i k + sigma_i eps, ending on alpha_end k + sigma_end eps -- on k itself
where the last row returns x_start (``denoise_to_zero``, ddim).  Not together with an x0 correction, which would rescale the held frames.
``plan_chunks`` cuts a long utterance into chunks that hold each other's last frames this way (``Denoiser.sample_long``).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

# column layout of the per-step coefficient table (float32, NCOEF per row)
COEF_COLUMNS = ("t_model", "alpha", "sigma", "g0", "g1", "A", "Bc", "d1c", "pc", "noise", "d2c", "pe")
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

    @classmethod
    def from_alphas_cumprod(cls, alphas_cumprod: np.ndarray) -> "VPSchedule":
        """the schedule of ``NoiseScheduleVP(alphas_cumprod=)`` (dpm_solver.py:104-105): log alpha = log(alphas_cumprod) / 2 in float32"""
        a32 = np.asarray(alphas_cumprod, dtype=np.float32).reshape(-1)
        s = cls(np.zeros(a32.shape[0], dtype=np.float32))
        s.log_alpha = (np.float32(0.5) * np.log(a32).astype(np.float32)).astype(np.float64)
        return s

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

    def timesteps(self, steps: int, t_T: float = 1.0, t_0: Optional[float] = None) -> np.ndarray:
        # the reference builds the grid with torch.linspace in float32
        return np.linspace(t_T, 1.0 / self.N if t_0 is None else t_0, steps + 1, dtype=np.float32).astype(np.float64)

    def inverse_lambda(self, lam: np.ndarray) -> np.ndarray:
        """t of a half-logSNR lambda (dpm_solver.py:156-167, discrete): log alpha = -logaddexp(0, -2 lambda) / 2, then the
        piecewise-linear inverse of log_alpha(t) over the same knots (extrapolated from the end segments, as interpolate_fn)"""
        la = -0.5 * np.logaddexp(0.0, -2.0 * np.asarray(lam, dtype=np.float64))
        xp, yp = self.log_alpha[::-1], self.knots[::-1]
        i = np.clip(np.searchsorted(xp, la, side="left") - 1, 0, self.N - 2)
        return yp[i] + (la - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])

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


SKIP_TYPES = ("logSNR", "time_uniform", "time_quadratic")
# the keyword-only options of build_table and their defaults (the settings the reference's model.py hard-codes): callers
# (Engine.load_sampler, Denoiser.sample, GroupedConverter, ...) pass them through unchanged and key their table caches on them
TABLE_OPTIONS = {"skip_type": "time_uniform", "lower_order_final": True, "denoise_to_zero": False, "variant": "bh2",
                 "solver_type": "dpmsolver", "t_start": None, "t_end": None, "method": "multistep"}


def table_options(opts: Dict[str, object]) -> Tuple[Tuple[str, object], ...]:
    """``opts`` checked against TABLE_OPTIONS -> a hashable cache key (options at their default left out)"""
    bad = sorted(set(opts) - set(TABLE_OPTIONS))
    if bad:
        raise TypeError(f"unknown sampler option(s) {bad}; known: {sorted(TABLE_OPTIONS)}")
    return tuple(sorted((k, v) for k, v in opts.items() if v != TABLE_OPTIONS[k] or type(v) is not type(TABLE_OPTIONS[k])))


def _grid_f32(sched: VPSchedule, skip_type: str, t_T: float, t_0: float, steps: int) -> np.ndarray:
    """the logSNR and time_quadratic grids as get_time_steps computes them (dpm_solver.py:453-479): float32 torch throughout,
    the logSNR end points through ``.item()``.  (A float64 logSNR grid moves the final latent by ~1e-5.)"""
    import torch
    f = torch.float32
    if skip_type == "time_quadratic":
        return torch.linspace(t_T ** 0.5, t_0 ** 0.5, steps + 1).pow(2).to(torch.float64).numpy()
    xs = torch.from_numpy(sched.knots.astype(np.float32))
    ys = torch.from_numpy(sched.log_alpha.astype(np.float32))

    def interp(x, xp, yp):        # interpolate_fn (dpm_solver.py:1241-1285): piecewise linear, end segments extrapolated
        i = torch.clamp(torch.searchsorted(xp, x) - 1, 0, xp.shape[0] - 2)
        return yp[i] + (x - xp[i]) * (yp[i + 1] - yp[i]) / (xp[i + 1] - xp[i])

    def lam(t):                   # marginal_lambda
        la = interp(torch.tensor([t], dtype=f), xs, ys)
        return (la - 0.5 * torch.log(1.0 - torch.exp(2.0 * la))).item()

    lams = torch.linspace(lam(t_T), lam(t_0), steps + 1)
    la = -0.5 * torch.logaddexp(torch.zeros((1,), dtype=f), -2.0 * lams)      # inverse_lambda
    return interp(la, torch.flip(ys, [0]), torch.flip(xs, [0])).to(torch.float64).numpy()


def build_table(solver: str, steps: int, betas: Optional[np.ndarray] = None, order: int = 2, eta: float = 0.0, *,
                skip_type: str = "time_uniform", lower_order_final: bool = True, denoise_to_zero: bool = False, variant: str = "bh2",
                solver_type: str = "dpmsolver", t_start: Optional[float] = None, t_end: Optional[float] = None,
                method: str = "multistep") -> SolverTable:
    """Coefficient table for ``steps`` denoiser evaluations (NFE == steps; ``denoise_to_zero``: steps + 1 evaluations and rows).

    ``unipc`` / ``dpmsolver++`` take the keyword options of the reference's ``UniPC.sample`` / ``DPM_Solver.sample``
    (uni_pc.py:590, dpm_solver.py:1047) that a captured loop can serve: ``order`` 1-3, ``skip_type`` (SKIP_TYPES),
    ``lower_order_final``, ``denoise_to_zero``, ``t_start`` / ``t_end`` (default T = 1 and 1/N), ``variant`` (UniPC: ``bh1`` |
    ``bh2``) and ``solver_type`` (DPM-Solver++ order 2: ``dpmsolver`` | ``taylor``).  ``method`` must be ``multistep``.

    ``ddim`` / ``ddpm`` need ``betas``, the model's own discrete schedule (pass the float64 betas, e.g.
    ``linear_betas(n, np.float64)``, to reproduce the reference's float32 buffers bit for bit); ``order`` and the keyword options
    do not apply to them.  ``eta`` is DDIM's noise scale (the reference's ``ddim_sampling_eta``); ``ddpm`` takes ``steps == len(betas)``."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    opts = dict(skip_type=skip_type, lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, variant=variant,
                solver_type=solver_type, t_start=t_start, t_end=t_end, method=method)
    if solver in DISCRETE_SOLVERS:
        given = table_options(opts)
        if given:
            raise ValueError(f"{solver} takes none of the continuous solvers' options, got {dict(given)}")
        return _discrete_table(solver, steps, betas, eta)
    if eta != 0.0:
        raise ValueError(f"eta applies to ddim only, not {solver!r}")
    if method != "multistep":
        raise ValueError(f"method must be 'multistep' (singlestep / adaptive solvers are not served by the captured loop), got {method!r}")
    if order not in (1, 2, 3):
        raise ValueError(f"order must be 1, 2 or 3, got {order!r}")
    if steps < order:
        raise ValueError(f"steps ({steps}) must be >= order ({order})")   # dpm_solver.py:1172 / uni_pc.py:607
    if skip_type not in SKIP_TYPES:
        raise ValueError(f"skip_type must be one of {SKIP_TYPES}, got {skip_type!r}")
    if variant not in ("bh1", "bh2") or (solver != "unipc" and variant != "bh2"):
        raise ValueError(f"variant must be 'bh1' or 'bh2' (UniPC only; vary_coeff is not served), got {variant!r} for {solver!r}")
    if solver_type not in ("dpmsolver", "taylor") or (solver != "dpmsolver++" and solver_type != "dpmsolver"):
        raise ValueError(f"solver_type must be 'dpmsolver' or 'taylor' (DPM-Solver++ only), got {solver_type!r} for {solver!r}")
    sched = betas if isinstance(betas, VPSchedule) else VPSchedule(linear_betas() if betas is None else betas)      # (a ready schedule: sampler/)
    t_T = 1.0 if t_start is None else float(t_start)
    t_0 = 1.0 / sched.N if t_end is None else float(t_end)
    if not 0.0 < t_0 < t_T <= 1.0:
        raise ValueError(f"need 0 < t_end < t_start <= 1, got t_start={t_T}, t_end={t_0}")
    ts = sched.timesteps(steps, t_T, t_0) if skip_type == "time_uniform" else _grid_f32(sched, skip_type, t_T, t_0, steps)
    lam = np.array([sched.lam(t) for t in ts])
    alpha = np.array([sched.alpha(t) for t in ts])
    sigma = np.array([sched.sigma(t) for t in ts])
    rows = steps + 1 if denoise_to_zero else steps
    coef = np.zeros((rows, NCOEF), dtype=np.float64)
    det = {k: np.zeros(steps + 1) for k in ("h", "rk", "B_h", "rho0", "rho1", "order")}
    unipc = solver == "unipc"

    def step_order(k: int) -> int:
        """order of the update that lands on ts[k], k = 1..steps"""
        if k < order:
            return k
        if lower_order_final and (unipc or steps < 10):        # uni_pc.py:636-637 (any steps) / dpm_solver.py:1198-1201 (< 10)
            return min(order, steps + 1 - k)
        return order

    def unipc_rhos(k: int, so: int):
        """B_h and the UniPC-bh rhos of update k at order so >= 2 (uni_pc.py:499-541): rk, rhos_p, rhos_c"""
        h = lam[k] - lam[k - 1]
        hh = -h
        h_phi_1 = np.expm1(hh)
        B_h = np.expm1(hh) if variant == "bh2" else hh
        rks = [(lam[k - 1 - j] - lam[k - 1]) / h for j in range(1, so)] + [1.0]
        b, h_phi_k, fac = [], h_phi_1 / hh - 1.0, 1
        for i in range(1, so + 1):
            b.append(h_phi_k * fac / B_h)
            fac *= i + 1
            h_phi_k = h_phi_k / hh - 1.0 / fac
        R = np.array([[r ** (i - 1) for r in rks] for i in range(1, so + 1)])
        rc = np.linalg.solve(R, np.array(b))
        rp = np.linalg.solve(R[:-1, :-1], np.array(b[:-1])) if so == 3 else np.array([0.5])
        return B_h, rks, rp, rc

    prev_pc = 0.0
    for i in range(steps):
        row = coef[i]
        row[0] = sched.model_time(ts[i])
        row[1], row[2] = alpha[i], sigma[i]
        # ---- correction of the state at t_i (uses the update that landed on ts[i])
        if i == 0:
            row[3] = row[4] = 0.0
        elif not unipc:
            row[3], row[4] = prev_pc, 0.0
        else:
            k = i
            so = step_order(k)
            if so <= 2:
                h = lam[k] - lam[k - 1]
                hh = -h
                h_phi_1 = np.expm1(hh)
                B_h = np.expm1(hh) if variant == "bh2" else hh
                if so == 1:
                    rho0, rho1 = 0.0, 0.5                        # uni_pc.py:541-542
                else:
                    rk = (lam[k - 2] - lam[k - 1]) / h
                    h_phi_k = h_phi_1 / hh - 1.0
                    b0 = h_phi_k / B_h
                    b1 = (h_phi_k / hh - 0.5) * 2.0 / B_h
                    rho0, rho1 = np.linalg.solve(np.array([[1.0, 1.0], [rk, 1.0]]), np.array([b0, b1]))   # :544
            else:
                B_h, _, _, rc = unipc_rhos(k, 3)
                rho0, rho1 = rc[0], rc[2]                        # rc_1 went into d1 (d2c of row k-1)
            ab = alpha[k] * B_h
            row[3], row[4] = ab * rho0, ab * rho1
            det["rho0"][k], det["rho1"][k] = rho0, rho1
        # ---- move towards t_{i+1}
        k = i + 1
        h = lam[k] - lam[k - 1]
        phi = np.expm1(-h)                                       # = h_phi_1 = B_h (bh2) with hh = -h
        so = step_order(k)
        row[5] = sigma[k] / sigma[k - 1]
        row[6] = alpha[k] * phi
        B_h = phi if (not unipc or variant == "bh2") else -h
        det["h"][k], det["B_h"][k], det["order"][k] = h, B_h, so
        if so == 2:
            rk = (lam[k - 2] - lam[k - 1]) / h                   # = -r0 of dpm_solver.py:822
            row[7] = 1.0 / rk
            if not unipc and solver_type == "taylor":
                row[8] = -alpha[k] * (phi / h + 1.0)             # dpm_solver.py:826-829
            else:
                row[8] = 0.5 * alpha[k] * B_h
            det["rk"][k] = rk
        elif so == 3 and unipc:
            B_h, rks, rp, rc = unipc_rhos(k, 3)
            ab = alpha[k] * B_h
            row[7] = 1.0 / rks[0]
            row[10] = (rc[1] / rc[0]) / rks[1]
            row[8] = ab * rp[0]
            row[11] = ab * rp[1] / rks[1] - row[8] * row[10]
            det["rk"][k] = rks[0]
        elif so == 3:
            # dpm_solver.py:871-889 with u = m_prev - m = -(model_prev_0 - model_prev_1), v = m_prev2 - m:
            # D1_0 = -u/r0, D1_1 = (u - v)/r1, x_t = xbar' + a*phi2*D1 - a*phi3*D2 = xbar' + c_u*u + c_v*v
            r0 = (lam[k - 1] - lam[k - 2]) / h
            r1 = (lam[k - 2] - lam[k - 3]) / h
            phi2 = phi / h + 1.0
            phi3 = phi2 / h - 0.5

            def x_minus_xbar(u, v):
                d10, d11 = -u / r0, (u - v) / r1
                D1 = d10 + (r0 / (r0 + r1)) * (d10 - d11)
                D2 = (1.0 / (r0 + r1)) * (d10 - d11)
                return alpha[k] * phi2 * D1 - alpha[k] * phi3 * D2

            c_u, c_v = x_minus_xbar(1.0, 0.0), x_minus_xbar(0.0, 1.0)
            row[8] = 0.5 * alpha[k] * phi
            row[7] = -c_u / row[8]
            row[10] = -c_v / row[8]
            det["rk"][k] = -r0
        else:
            row[7] = row[8] = 0.0
        prev_pc = row[8]
    if denoise_to_zero:              # uni_pc.py:660-665 / dpm_solver.py:1228-1233: x_start of one more evaluation at t_0
        row = coef[steps]
        t0 = float(np.float32(t_0))
        row[0] = sched.model_time(t0)
        row[1], row[2] = sched.alpha(t0), sched.sigma(t0)
        row[5], row[6] = 0.0, -1.0
    return SolverTable(solver, rows, coef.astype(np.float32), ts, det)


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


SCHEDULE_KEYS = ("solver", "steps", "order", "eta") + tuple(TABLE_OPTIONS)      # the keys of one item's schedule (a dict)


def schedule_key(spec: Dict[str, object], item: Optional[int] = None) -> Tuple:
    """One item's schedule -- ``dict(solver=, steps=, order=2, eta=0.0, **table options)`` -- checked and made hashable:
    ``(solver, steps, order, eta, table_options)``.  Equal schedules have equal keys.  ``item`` names the item in the error."""
    who = "schedule" if item is None else f"schedules[{item}]"
    if not isinstance(spec, dict):
        raise ValueError(f"{who} must be a dict with the keys {SCHEDULE_KEYS[:4]} and the table options, got {type(spec).__name__}")
    bad = sorted(set(spec) - set(SCHEDULE_KEYS))
    if bad:
        raise ValueError(f"{who}: unknown key(s) {bad}; known: {list(SCHEDULE_KEYS)}")
    if spec.get("solver") not in SOLVERS:
        raise ValueError(f"{who}: solver must be one of {SOLVERS}, got {spec.get('solver')!r}")
    if not isinstance(spec.get("steps"), (int, np.integer)) or isinstance(spec.get("steps"), bool) or int(spec["steps"]) <= 0:
        raise ValueError(f"{who}: steps must be a positive int, got {spec.get('steps')!r}")
    opts = {k: v for k, v in spec.items() if k in TABLE_OPTIONS}
    if opts.get("method", "multistep") != "multistep":
        raise ValueError(f"{who}: method must be 'multistep' (singlestep / adaptive solvers are not served by the captured loop), got {opts['method']!r}")
    return (spec["solver"], int(spec["steps"]), int(spec.get("order", 2)), float(spec.get("eta", 0.0)), table_options(opts))


@dataclass
class ItemTables:
    """The per-item schedules of one batch (``build_tables``): the DISTINCT tables, and per loop item which of them it walks and the loop
    step it starts at.  The loop runs ``steps`` = max(start + rows) steps; ``row_at(r)`` / ``t_model_at(r)`` give every item's table row
    (clamped for a held item) and model time at loop step r, ``active_at(r)`` who is updated there."""
    tables: List[SolverTable]
    index: np.ndarray         # (B,) int32: item b walks tables[index[b]]
    start: np.ndarray         # (B,) int32
    keys: Tuple = ()

    @property
    def rows(self) -> np.ndarray:
        return np.array([t.steps for t in self.tables], dtype=np.int32)

    @property
    def item_rows(self) -> np.ndarray:
        return self.rows[self.index]

    @property
    def steps(self) -> int:
        return int((self.start + self.item_rows).max())

    @property
    def coef(self) -> np.ndarray:
        """the rows of the distinct tables back to back, (sum(rows), NCOEF) float32: what the engine's device table holds"""
        return np.ascontiguousarray(np.concatenate([np.asarray(t.coef, dtype=np.float32) for t in self.tables], axis=0))

    def row_at(self, r: int) -> np.ndarray:
        return np.clip(int(r) - self.start, 0, self.item_rows - 1).astype(np.int32)

    def active_at(self, r: int) -> np.ndarray:
        j = int(r) - self.start
        return (j >= 0) & (j < self.item_rows)

    def t_model_at(self, r: int) -> np.ndarray:
        j = self.row_at(r)
        return np.array([self.tables[k].coef[j[b], 0] for b, k in enumerate(self.index)], dtype=np.float32)

    def table_of(self, b: int) -> SolverTable:
        return self.tables[int(self.index[b])]

    @property
    def uniform(self) -> bool:
        """every item walks the same table: the shared-table loop serves the batch"""
        return len(self.tables) == 1


def build_tables(specs, betas: Optional[np.ndarray] = None, discrete_betas: Optional[np.ndarray] = None, starts=None) -> ItemTables:
    """One schedule per loop item (``schedule_key`` states the dict) -> ``ItemTables``.  Equal schedules share one table (and its rows in
    the engine).  ``betas``: the continuous solvers' schedule as ``build_table`` takes it; ``discrete_betas``: ddim / ddpm's (the model's
    float64 betas; default ``betas``).  Items are RIGHT-ALIGNED, start_b = S - rows_b with S the longest table: all finish together, so
    the last k loop steps are every item's last min(k, rows_b) evaluations -- what a mixed-precision tail needs.  ``starts`` overrides that
    (the engine takes any start >= 0)."""
    specs = list(specs)
    if not specs:
        raise ValueError("build_tables needs at least one schedule")
    keys = [schedule_key(s, b) for b, s in enumerate(specs)]
    distinct: Dict[Tuple, int] = {}
    tables: List[SolverTable] = []
    index = np.zeros((len(keys),), dtype=np.int32)
    for b, key in enumerate(keys):
        if key not in distinct:
            solver, steps, order, eta, opts = key
            try:
                tables.append(build_table(solver, steps, (discrete_betas if discrete_betas is not None else betas) if solver in DISCRETE_SOLVERS else betas,
                                          order, eta, **dict(opts)))
            except ValueError as e:
                raise ValueError(f"schedules[{b}]: {e}") from None
            distinct[key] = len(tables) - 1
        index[b] = distinct[key]
    rows = np.array([t.steps for t in tables], dtype=np.int32)[index]
    if starts is None:
        start = (rows.max() - rows).astype(np.int32)
    else:
        start = np.ascontiguousarray(np.asarray(starts).reshape(-1), dtype=np.int32)
        if start.shape[0] != len(keys) or (start < 0).any():
            raise ValueError(f"starts must hold one loop step >= 0 per item ({len(keys)})")
    return ItemTables(tables, index, start, tuple(keys))


# ---- the host statement of the sampler: ``solver_update`` states the recurrence, the three loops below drive it -----------------
def solver_update(c, hist2: bool, x0, xe, xbar, d1, m_prev, m_prev2, correct: Optional[Dict[str, object]] = None, z=None):
    """The update of ONE table row in float32, on state arrays of any leading shape: the host twin of common.h ``solver_elem`` + ``solver_xe``
    and the only place where this module evaluates the recurrence of its docstring.  ``c``: the row (NCOEF columns); ``x0``: what the model
    returned at ``xe`` (after guidance and hold).  ``hist2``: the item's TABLE has a row of order 3 (``has_history2``) -- a property of the
    table, not of the row: every row of such a table takes the history-2 expressions and rotates ``m_prev2``, also one whose columns 10-11
    are zero.  ``correct``: None or the keywords of ``correct_x0``, applied to m before anything reads it.  ``z``: standard normals shaped
    like the state, read only where the row's noise column is not zero (a zero coefficient adds no term at all).
    Returns the new ``(xe, xbar, d1, m_prev, m_prev2)`` as fresh arrays -- except ``m_prev2``, which is the ``m_prev`` it was given (history
    2) or the ``m_prev2`` it was given (otherwise): a caller that writes the result back into those buffers stores ``m_prev2`` first."""
    f = np.float32
    _, alpha, sigma, g0, g1, A, Bc, d1c, pc = (f(v) for v in c[:9])
    eps = (xe - alpha * x0) / sigma
    m = (xe - sigma * eps) / alpha
    if correct is not None:
        m = _correct_x0(m, **correct)
    x = xbar - g0 * d1 - g1 * (m - m_prev)
    xbar = A * x - Bc * m
    if c[9] != 0:
        xbar = xbar + f(c[9]) * z
    if hist2:
        d2c, pe = f(c[10]), f(c[11])
        d1 = d1c * (m_prev - m) + d2c * (m_prev2 - m)
        xe = xbar - pc * d1 - pe * (m_prev2 - m)
        m_prev2 = m_prev
    else:
        d1 = d1c * (m_prev - m)
        xe = xbar - pc * d1
    return xe, xbar, d1, m, m_prev2


def _start_state(x_T: np.ndarray) -> List[np.ndarray]:
    """the state in front of the first evaluation, [xe, xbar, d1, m_prev, m_prev2] = [x_T, x_T, 0, 0, 0]: five buffers of their own"""
    return [x_T.copy(), x_T.copy()] + [np.zeros_like(x_T) for _ in range(3)]


def _loop_correction(correct_x0) -> Optional[Dict[str, object]]:
    """a loop's ``correct_x0=`` dict checked (ValueError) -> a copy of it, or None where the correction is off"""
    if correct_x0 is not None and check_x0_correction(correct_x0.get("mode"), correct_x0.get("ratio", 0.995), correct_x0.get("max_val", 1.0)):
        return dict(correct_x0)
    return None


def _item_step(state, b: int, x0, table: SolverTable, j: int, hist2: bool, corr, own, noise_fn, noise_key, who: str) -> None:
    """Row j of ``table`` on item b of the state of a per-item loop (``run_tables_numpy``, ``run_slots_numpy``), in place.  Its correction: the
    loop-wide ``corr`` under ``lengths[b]``, else the item's ``own`` entry; its normals: ``noise_fn(*noise_key)``, shaped like one item."""
    c = table.coef[j]
    correct = own
    if corr is not None:
        lengths = corr.get("lengths")
        correct = dict(corr, lengths=None if lengths is None else [lengths[b]])
    z = None
    if c[9] != 0:
        if noise_fn is None:
            raise ValueError(f"row {j} of {who}'s {table.solver} table adds noise: pass noise_fn")
        z = np.asarray(noise_fn(*noise_key), dtype=np.float32)[None]
    sl = slice(b, b + 1)
    new = solver_update(c, hist2, x0[sl], *(a[sl] for a in state), correct, z)
    for a, v in zip(reversed(state), reversed(new)):      # (m_prev2 may be the view of m_prev: stored before m_prev is)
        a[sl] = v


def run_tables_numpy(tabs: ItemTables, x0_fn: Callable[[np.ndarray, np.ndarray], np.ndarray], x_T: np.ndarray,
                     trace: Optional[List[np.ndarray]] = None, noise_fn: Optional[Callable[[int, int], np.ndarray]] = None,
                     guided_x0: Optional[np.ndarray] = None, correct_x0: Optional[Dict[str, object]] = None, hold=None) -> np.ndarray:
    """Host statement of the loop under per-item schedules (float32).  At loop step r item b has j = r - start_b: ACTIVE when
    0 <= j < rows_b -- it then takes row j of its own table through ``solver_update`` (``_item_step``), history 2 where ITS table has a
    nonzero column 10 or 11 --, otherwise HELD: evaluated at the clamped row's model time, result ignored, state untouched.
    ``x0_fn(x (B, ...), t_model (B,)) -> x0`` sees every item's own model time.  ``noise_fn(b, j)`` -> the standard normals of item b at
    its LOCAL row j, shaped like x_T[b] (``noise.gauss(seed_b, j, ...)``: the stream the item has alone).  ``guided_x0``: (B,) scales --
    ``x0_fn`` is then called on cat([x, x]) and cat([t, t]) (unconditional half first) and the halves are combined by
    ``schedule.guided_x0``.  ``correct_x0``: the keywords of ``schedule.correct_x0`` for the whole batch (``lengths`` per item); refused when
    an item is stochastic.  A LIST instead is the per-item correction: one entry per item, None or such a dict for that item
    alone (``lengths`` = its own frame count; ``item_correction``); item b is then corrected exactly as ``run_table_numpy(correct_x0=entry_b)``
    corrects it alone, a stochastic item takes None, and corrected and stochastic items may share the batch.
    ``hold`` = (known, mask): known frames as in ``run_table_numpy`` -- applied at every loop step, also to an item its schedule holds there
    (its x0 is ignored at that step anyway); not together with ``correct_x0``."""
    f = np.float32
    B = x_T.shape[0]
    hold = _check_hold(hold, x_T.shape, correct_x0)
    if tabs.index.shape[0] != B:
        raise ValueError(f"{tabs.index.shape[0]} schedules for a batch of {B}")
    state = _start_state(x_T.astype(f))
    xe = state[0]
    hist2 = [has_history2(tabs.table_of(b)) for b in range(B)]
    noisy = [bool((np.asarray(tabs.table_of(b).coef)[:, 9] != 0).any()) for b in range(B)]
    corr = None
    per_item = [None] * B
    if isinstance(correct_x0, (list, tuple)):
        per_item = item_corrections(correct_x0, B, noisy)
    else:
        corr = _loop_correction(correct_x0)
        if corr is not None and any(noisy):
            raise ValueError(f"the x0 correction does not apply to a batch with a stochastic item (items {[b for b in range(B) if noisy[b]]})")
    for r in range(tabs.steps):
        t = tabs.t_model_at(r)
        if guided_x0 is None:
            x0 = np.asarray(x0_fn(xe, t)).astype(f)
        else:
            both = np.asarray(x0_fn(np.concatenate([xe, xe], axis=0), np.concatenate([t, t]))).astype(f)
            x0 = _guided_x0(both[:B], both[B:], np.asarray(guided_x0, dtype=f))
        x0 = hold_x0(x0, hold)
        rows, act = tabs.row_at(r), tabs.active_at(r)
        for b in range(B):
            if act[b]:
                _item_step(state, b, x0, tabs.table_of(b), int(rows[b]), hist2[b], corr, per_item[b], noise_fn, (b, int(rows[b])), f"item {b}")
        if trace is not None:
            trace.append(xe.copy())
    return xe


def guided_x0(x0_u: np.ndarray, x0_c: np.ndarray, scale) -> np.ndarray:
    """Classifier-free guidance, the host statement of common.h ``guided_x0``: ``x0_u + s * (x0_c - x0_u)`` per item, ``scale`` a float or
    (B,) against (B, ...) arrays.  The reference combines in noise space (sampler/uni_pc.py:225-229, sampler/dpm_solver.py:327-331); with the
    x_start wrapper eps = (x - alpha x0) / sigma is affine in x0 with the same x, alpha, sigma in both halves, so this is the same point.
    Where ``scale == 1`` the result IS ``x0_c`` by a select (not ``x0_u + 1 * (x0_c - x0_u)``): such an item takes nothing from ``x0_u``
    -- no rounding, no NaN -- and follows its unguided trajectory (the reference's short cut, uni_pc.py:222-223, per item)."""
    x0_u, x0_c = np.asarray(x0_u), np.asarray(x0_c)
    s = np.asarray(scale, dtype=x0_c.dtype)
    if s.ndim > 1 or (s.ndim == 1 and s.shape[0] != x0_c.shape[0]):
        raise ValueError(f"scale must be a float or hold one scale per item ({x0_c.shape[0]},), got shape {s.shape}")
    s = s.reshape(s.shape + (1,) * (x0_c.ndim - s.ndim)) if s.ndim else s
    with np.errstate(invalid="ignore"):
        return np.where(s == 1, x0_c, x0_u + s * (x0_c - x0_u)).astype(x0_c.dtype)


_guided_x0 = guided_x0      # (run_tables_numpy has a keyword of that name)
X0_CORRECTIONS = {None: 0, "dynamic_thresholding": 1, "clamp": 2}      # Denoiser.sample(correcting_x0_fn=) -> the engine's mode


def abs_quantile(a: np.ndarray, p: float) -> np.float32:
    """``torch.quantile(|a|.reshape(-1), p)`` of a float32 array, bit for bit: linear interpolation between the ascending order statistics
    evaluated in float32 -- pos = f32(p) * f32(n - 1), lo = floor(pos), hi = ceil(pos), w = pos - lo -- and torch's own lerp, a fused
    multiply-add from the nearer end: v_lo + w (v_hi - v_lo) where w < 0.5, v_hi - (v_hi - v_lo)(1 - w) otherwise.  The engine's radix
    select (misc.hip abs_quantile_kernel) finds the same v_lo, v_hi and evaluates the same expression."""
    f = np.float32
    v = np.sort(np.abs(np.asarray(a, dtype=f)).reshape(-1))
    n = v.shape[0]
    if n == 0:
        raise ValueError("abs_quantile of an empty array")
    if not 0.0 <= float(p) <= 1.0:
        raise ValueError(f"p must be in [0, 1], got {p}")
    pos = f(p) * f(n - 1)
    lo, hi = int(np.floor(pos)), int(np.ceil(pos))
    w = f(pos - f(lo))
    d = np.float64(f(v[hi] - v[lo]))      # (the product of two float32 is exact in float64: one rounding, as the fused form)
    if w < f(0.5):
        return f(np.float64(w) * d + np.float64(v[lo]))
    return f(np.float64(v[hi]) - d * np.float64(f(f(1) - w)))


def check_x0_correction(mode, ratio: float = 0.995, max_val: float = 1.0, names_only: bool = False) -> int:
    """the argument errors of the x0 correction (ValueError); ``mode`` None | "dynamic_thresholding" | "clamp" -> 0 | 1 | 2.  The engine's own
    numbers 0 | 1 | 2 are accepted too (``Engine.set_x0_correction``, ``correct_x0``) unless ``names_only``: the public keyword
    ``correcting_x0_fn`` of ``Denoiser.sample`` and the classes around it takes the names alone."""
    if callable(mode):
        raise ValueError("correcting_x0_fn: a callable cannot run inside the captured loop; pass 'dynamic_thresholding', 'clamp' or None")
    if not names_only and isinstance(mode, (int, np.integer)) and not isinstance(mode, bool) and int(mode) in (0, 1, 2):
        m = int(mode)
    elif mode is None or isinstance(mode, str) and mode in X0_CORRECTIONS:
        m = X0_CORRECTIONS[mode]
    else:
        raise ValueError(f"correcting_x0_fn must be None, 'dynamic_thresholding' or 'clamp', got {mode!r}")
    try:
        r, v = float(ratio), float(max_val)
    except (TypeError, ValueError):
        raise ValueError(f"dynamic_thresholding_ratio and thresholding_max_val must be numbers, got {ratio!r}, {max_val!r}") from None
    if not 0.0 <= r <= 1.0:      # (NaN fails both comparisons)
        raise ValueError(f"dynamic_thresholding_ratio must be in [0, 1], got {ratio!r}")
    if not (np.isfinite(v) and v > 0.0):
        raise ValueError(f"thresholding_max_val must be finite and > 0, got {max_val!r}")
    return m


def correct_x0(m: np.ndarray, mode, ratio: float = 0.995, max_val: float = 1.0, lengths=None) -> np.ndarray:
    """The reference's correction of the predicted x0 (sampler/dpm_solver.py:416-425, :433-442, sampler/uni_pc.py:268-294), float32, on
    ``m`` (B, C, T) -- the model value after the x_start round trip.  ``dynamic_thresholding``: per item s = max(abs_quantile(m_b, ratio),
    max_val), clamp(m_b, -s, s) / s, the quantile over the item's own frames t < lengths[b] (all T without lengths: what the reference
    computes for the item alone at T = lengths[b]).  ``clamp``: clamp(m, -max_val, max_val).  The frames past an item's end pass through
    the same clamp (zeros stay zeros)."""
    mode = check_x0_correction(mode, ratio, max_val)
    f = np.float32
    m = np.asarray(m, dtype=f)
    if mode == 0:
        return m
    if mode == 2:
        return np.clip(m, f(-max_val), f(max_val))
    out = np.empty_like(m)
    for b in range(m.shape[0]):
        L = m.shape[-1] if lengths is None else int(lengths[b])
        s = max(abs_quantile(m[b, ..., :L], ratio), f(max_val))
        out[b] = np.clip(m[b], -s, s) / s
    return out


_correct_x0 = correct_x0      # (run_table_numpy has a keyword of that name)


def item_correction(c, noisy: bool = False, what: str = "item") -> Optional[Dict[str, object]]:
    """One item's entry of a per-item x0 correction -> the keywords of ``correct_x0`` for that item alone, or None where it is
    off.  ``c``: None or ``dict(mode=, ratio=, max_val=, lengths=)`` as ``run_table_numpy(correct_x0=)`` takes it, ``lengths`` the item's
    own frame count (a number or a one-entry list).  A stochastic item (``noisy``) takes None or mode 0 alone."""
    if c is None:
        return None
    if not isinstance(c, dict):
        raise ValueError(f"{what}: a per-item x0 correction is None or a dict(mode=, ratio=, max_val=, lengths=), got {c!r}")
    extra = set(c) - {"mode", "ratio", "max_val", "lengths"}
    if extra:
        raise ValueError(f"{what}: unknown x0 correction keys {sorted(extra)}")
    mode = check_x0_correction(c.get("mode"), c.get("ratio", 0.995), c.get("max_val", 1.0))
    if mode == 0:
        return None
    if noisy:
        raise ValueError(f"{what} is stochastic and asks for an x0 correction: ddim / ddpm have no correction")
    L = c.get("lengths")
    if L is not None:
        L = [int(np.asarray(L).reshape(-1)[0])] if np.asarray(L).size == 1 else None
        if L is None:
            raise ValueError(f"{what}: lengths of a per-item x0 correction is the item's own frame count")
    return dict(mode=mode, ratio=float(c.get("ratio", 0.995)), max_val=float(c.get("max_val", 1.0)), lengths=L)


def item_corrections(entries, n: int, noisy: Optional[Sequence[bool]] = None) -> List[Optional[Dict[str, object]]]:
    """``item_correction`` of a list of ``n`` entries (ValueError on another length); ``noisy[b]``: item b is stochastic"""
    if len(entries) != n:
        raise ValueError(f"{len(entries)} per-item x0 corrections for {n} items")
    return [item_correction(c, bool(noisy[b]) if noisy is not None else False, f"item {b}") for b, c in enumerate(entries)]


# ---- known frames -----------------------------------------------------------------------------------------
def _check_hold(hold, shape, correct_x0=None):
    """``hold`` = None or (known, mask) -> None or (known float32 shaped ``shape`` = (B, C, T), mask (B, T) bool); ValueError otherwise"""
    if hold is None:
        return None
    if not isinstance(hold, (tuple, list)) or len(hold) != 2 or hold[0] is None or hold[1] is None:
        raise ValueError("hold is a pair (known, mask): the known latent and the frame mask are given together")
    if correct_x0 is not None:
        raise ValueError("known frames (hold=) do not run with an x0 correction (correct_x0=): it would rescale the held frames")
    known, mask = np.asarray(hold[0], dtype=np.float32), np.asarray(hold[1])
    if known.shape != tuple(shape):
        raise ValueError(f"known must be shaped like x_T {tuple(shape)}, got {known.shape}")
    if mask.shape != (shape[0], shape[-1]) or mask.dtype != np.bool_:
        raise ValueError(f"the known-frame mask must be a bool array ({shape[0]}, {shape[-1]}), got {mask.dtype} {mask.shape}")
    return known, mask


def hold_x0(x0: np.ndarray, hold) -> np.ndarray:
    """the engine's hold launch on the host: ``known`` on the masked frames of x0 (B, C, T), every other element unchanged; ``hold`` None: x0"""
    if hold is None:
        return x0
    known, mask = hold
    return np.where(mask[:, None, :], known, x0).astype(np.float32)


def known_start(x_T: np.ndarray, known: np.ndarray, mask: np.ndarray, coef_row0) -> np.ndarray:
    """The start state of a loop with known frames (float32): ``alpha * known + sigma * x_T`` on the masked frames, x_T elsewhere, with
    alpha and sigma the float32 columns 1 and 2 of the item's first table row -- ``coef_row0`` is that row (NCOEF,), shared, or (B, NCOEF), one
    per item (per-item schedules: each item's own row 0).  A held frame then stays on the forward marginal of ``known`` with the noise
    x_T[b, :, t] all the way: x_i = alpha_i k + sigma_i eps."""
    f = np.float32
    x_T = np.asarray(x_T, dtype=f)
    known, mask = _check_hold((known, mask), x_T.shape)
    row = np.asarray(coef_row0, dtype=f)
    if row.shape not in ((NCOEF,), (x_T.shape[0], NCOEF)):
        raise ValueError(f"coef_row0 must be one table row ({NCOEF},) or one per item ({x_T.shape[0]}, {NCOEF}), got {row.shape}")
    a = row[..., 1].reshape((-1,) + (1,) * (x_T.ndim - 1))
    s = row[..., 2].reshape((-1,) + (1,) * (x_T.ndim - 1))
    return np.where(mask[:, None, :], (a * known).astype(f) + (s * x_T).astype(f), x_T).astype(f)


def known_start_torch(x_T, known, mask: np.ndarray, coef_row0):
    """``known_start`` on float32 torch tensors (B, C, T) of one device, for the engine's callers: ``mask`` is the host bool array (B, T),
    ``coef_row0`` one table row or one per item as above.  The arguments are the caller's checked ones; nothing is checked again."""
    import torch
    B, _, T = x_T.shape
    row = np.asarray(coef_row0, dtype=np.float32)
    a0, s0 = (torch.from_numpy(np.array(np.broadcast_to(row[..., k], (B,)))).to(x_T.device).view(B, 1, 1) for k in (1, 2))
    return torch.where(torch.from_numpy(mask).to(x_T.device).view(B, 1, T), a0 * known + s0 * x_T, x_T).contiguous()


def plan_chunks(length: int, chunk_frames: int, overlap_frames: int) -> List[Tuple[int, int]]:
    """The chunks [(start, stop)] that ``Denoiser.sample_long`` cuts an utterance of ``length`` frames into: at most ``chunk_frames`` long,
    consecutive ones sharing exactly ``overlap_frames`` frames (0 <= overlap < chunk), which the later chunk holds as known frames.  The
    starts are j * (chunk - overlap) for as long as start + overlap < length -- every chunk adds at least one new frame -- and
    stop = min(start + chunk, length).  Chunk 0 always exists: an utterance no longer than the overlap is that one chunk."""
    L, C, V = int(length), int(chunk_frames), int(overlap_frames)
    if L < 1 or C < 1:
        raise ValueError(f"length and chunk_frames must be >= 1, got {length}, {chunk_frames}")
    if not 0 <= V < C:
        raise ValueError(f"overlap_frames must be in [0, chunk_frames), got {overlap_frames} of {chunk_frames}")
    out, start = [], 0
    while start == 0 or start + V < L:
        out.append((start, min(start + C, L)))
        start += C - V
    return out


def has_history2(table: SolverTable) -> bool:
    """the table needs m_prev2 (some row of order 3): what the engine's ns2vc_sampler_load detects from columns 10-11"""
    return bool((np.asarray(table.coef)[:, 10:12] != 0).any())


def run_table_numpy(table: SolverTable, x0_fn: Callable[[np.ndarray, np.ndarray], np.ndarray], x_T: np.ndarray,
                    trace: Optional[List[np.ndarray]] = None, noise_fn: Optional[Callable[[int], np.ndarray]] = None,
                    correct_x0: Optional[Dict[str, object]] = None, hold=None) -> np.ndarray:
    """Host executor of the unified recurrence (float32, one ``solver_update`` of the whole batch per row), used by CPU tests to pin
    the tables against the oracle samplers.  ``x0_fn(x, t_model[B]) -> x0``.  ``noise_fn(i)`` -> the standard normals of
    step i, shaped like x_T (ns2vc_amd.noise.gauss), for tables with a nonzero noise column.
    ``correct_x0``: None (off) or the keywords of ``schedule.correct_x0`` -- ``dict(mode=, ratio=, max_val=, lengths=)`` -- applied to m
    in front of everything that uses it (the reference's ``data_prediction_fn``); not together with a noise column.
    ``hold`` = (known, mask), the known frames of DESIGN 4.16: ``known`` shaped like x_T, ``mask`` (B, T) bool -- straight after ``x0_fn``,
    before anything reads its result, ``x0[b, :, t] = known[b, :, t]`` wherever ``mask[b, t]`` (``hold_x0``); every other element keeps its
    bits.  The update is linear in x0, so such a frame follows x_i = alpha_i k + sigma_i eps with the eps of its start state
    (``known_start``).  Not together with ``correct_x0``, which would rescale the held frames."""
    f = np.float32
    hold = _check_hold(hold, x_T.shape, correct_x0)
    state = _start_state(x_T.astype(f))
    hist2 = has_history2(table)
    B = x_T.shape[0]
    if _loop_correction(correct_x0) is not None and (np.asarray(table.coef)[:, 9] != 0).any():
        raise ValueError(f"the x0 correction does not apply to a stochastic {table.solver} table (the reference's discrete samplers have none)")
    for i in range(table.steps):
        c = table.coef[i]
        x0 = hold_x0(x0_fn(state[0], np.full((B,), f(c[0]), dtype=f)).astype(f), hold)
        z = None
        if c[9] != 0:
            if noise_fn is None:
                raise ValueError(f"step {i} of this {table.solver} table adds noise: pass noise_fn")
            z = np.asarray(noise_fn(i), dtype=f)
        state = solver_update(c, hist2, x0, *state, correct_x0, z)
        if trace is not None:
            trace.append(state[0].copy())
    return state[0]


# ---- slot loops: continuous batching ---------------------------------------------------------------------
TABLE_ROWS = 1024         # rows of the engine's coefficient table (its fixed capacity)
ITEM_HIST2, ITEM_NOISE = 1, 2      # record flags (common.h SOLVER_ITEM_*)


def table_flags(table: SolverTable) -> int:
    """the form an item with this table runs (the engine derives the same from the rows): 1 = history 2, 2 = noise"""
    c = np.asarray(table.coef)
    return (ITEM_HIST2 if (c[:, 10:12] != 0).any() else 0) | (ITEM_NOISE if (c[:, 9] != 0).any() else 0)


def run_slots_numpy(timeline, x0_fn: Callable[[np.ndarray, np.ndarray], np.ndarray], shape, trace: Optional[List[np.ndarray]] = None,
                    noise_fn: Optional[Callable[[int, int, int], np.ndarray]] = None, correct_x0: Optional[Dict[str, object]] = None):
    """Host statement of a slot loop (float32).  ``timeline[b]`` = the consecutive items of slot b, each ``(table, start, x_T)`` with
    ``x_T`` shaped ``shape[1:]`` and ``start`` >= the previous item's start + rows; ``shape`` = (B, ...) of the loop's state.  At loop step r
    the item of slot b with start <= r < start + rows is ACTIVE at its row r - start (``run_tables_numpy``'s ``_item_step``, history 2 where ITS
    table has it); at r == start its state is loaded from x_T first (x_e = x_bar = x_T, d1 = m_prev = m_prev2 = 0: what an admission
    writes).  A slot between items is HELD: evaluated -- at the clamped row of its last item, or at model time 0 while it has had none --,
    never updated.  ``x0_fn(x (B, ...), t (B,))`` must treat the items independently, as the engine does.  ``noise_fn(b, k, j)`` -> the
    normals of slot b's k-th item at its LOCAL row j.  Returns ``results[b][k]`` = x_e of that item after its last row: equal, bit for
    bit, to the item run alone (``run_table_numpy``).  ``correct_x0``: the keywords of ``schedule.correct_x0`` for every item of the loop.  A
    request's OWN correction is a fourth tuple element instead, ``(table, start, x_T, correction)``: None or the dict
    ``item_correction`` takes (``lengths`` = the item's own frame count); a stochastic item takes None; not together with ``correct_x0=``.
    A request's known frames are a fifth element, ``(table, start, x_T, correction, hold)``: None or ``(known, mask)`` shaped
    ``shape[1:]`` and ``(T,)`` bool.  ``hold_x0`` is applied to that slot's x0 at every evaluation while the item is the slot's current one --
    from its admission until the next one, as the engine's per-slot mask stands until the slot is taken -- so the item equals
    ``run_table_numpy(..., hold=)`` of it alone, bit for bit.  Refused together with a correction, in the same tuple or in ``correct_x0=``.
    A request run in PIECES (suspend and resume) is a sixth element, ``(table, start, x_T, correction, hold, (request, a, b))``:
    this entry runs rows ``[a, b)`` of the table, 0 <= a < b <= rows, at loop steps start .. start + (b - a) - 1.  ``request`` is any hashable
    name that the pieces of one request share; they may sit in the same slot or in different ones.  A piece with a == 0 loads its state from
    x_T as an admission does; a piece with a > 0 loads the five state arrays the piece of the same request that ended at row a left (that piece
    must have ended at an earlier loop step; its x_T is not read) -- what a resume writes.  A piece with b < rows saves the state after row
    b - 1 and has the result None -- what a suspend copies out; the piece with b == rows gives the request's result.  Correction and hold are
    sent with every piece, as the engine's caller sends them with every resume; ``noise_fn(b, k, j)`` gets the row j of the TABLE, so a
    stochastic request continues its own stream when it keys the stream by j.  The result equals ``run_table_numpy`` of the request alone."""
    f = np.float32
    B = int(shape[0])
    if len(timeline) != B:
        raise ValueError(f"{len(timeline)} slot timelines for {B} slots")

    def rows_of(item):      # the rows [a, b) of its table this timeline entry runs, and the request it is a piece of (None: a whole request)
        if len(item) > 5 and item[5] is not None:
            rid, a, e = item[5]
            if not 0 <= int(a) < int(e) <= item[0].steps:
                raise ValueError(f"a piece runs rows [a, b) with 0 <= a < b <= {item[0].steps}, got [{a}, {e})")
            return int(a), int(e), rid
        return 0, item[0].steps, None

    for b, items in enumerate(timeline):
        end = 0
        for k, item in enumerate(items):
            start = item[1]
            if int(start) < end:
                raise ValueError(f"slot {b}: item {k} starts at loop step {start}, the slot is busy until {end}")
            a, e, _ = rows_of(item)
            end = int(start) + e - a
    own = [[item_correction(item[3], bool(table_flags(item[0]) & ITEM_NOISE), f"slot {b} item {k}") if len(item) > 3 else None
            for k, item in enumerate(items)] for b, items in enumerate(timeline)]
    if correct_x0 is not None and any(len(item) > 3 for items in timeline for item in items):
        raise ValueError("run_slots_numpy: either correct_x0= for every item or a fourth tuple element per item, not both")
    corr = _loop_correction(correct_x0)
    holds = [[None] * len(items) for items in timeline]
    for b, items in enumerate(timeline):
        for k, item in enumerate(items):
            if len(item) > 4 and item[4] is not None:
                if item[3] is not None:
                    raise ValueError(f"slot {b} item {k}: known frames do not run with an x0 correction: it would rescale the held frames")
                h = item[4]
                if isinstance(h, (tuple, list)) and len(h) == 2 and h[0] is not None and h[1] is not None:
                    h = (np.asarray(h[0])[None], np.asarray(h[1])[None])      # (one item: the batch axis _check_hold expects)
                hk, hm = _check_hold(h, (1,) + tuple(shape[1:]))
                holds[b][k] = (hk[0], hm[0])
    state = _start_state(np.zeros(shape, f))
    xe = state[0]
    S = max([int(item[1]) + rows_of(item)[1] - rows_of(item)[0] for items in timeline for item in items], default=0)
    results = [[None] * len(items) for items in timeline]
    cur = [-1] * B          # the item slot b holds (the last one admitted)
    hist2 = [False] * B     # ... and whether its table has history 2
    saved: Dict[object, tuple] = {}      # request -> (rows run, its five state arrays) left by its last piece
    for r in range(S):
        t = np.zeros((B,), f)
        act = [None] * B
        for b, items in enumerate(timeline):
            if cur[b] + 1 < len(items) and int(items[cur[b] + 1][1]) == r:      # admission, or the resume of a later piece
                cur[b] += 1
                hist2[b] = has_history2(items[cur[b]][0])
                a0, _, rid = rows_of(items[cur[b]])
                if a0 > 0:
                    if rid not in saved or saved[rid][0] != a0:
                        raise ValueError(f"slot {b} item {cur[b]}: no piece of request {rid!r} has ended at row {a0} before loop step {r}")
                    first = saved.pop(rid)[1]
                else:
                    first = _start_state(np.asarray(items[cur[b]][2], dtype=f))
                for a, v in zip(state, first):
                    a[b] = v
            if cur[b] >= 0:
                tab, start = items[cur[b]][0], items[cur[b]][1]
                a0, e0, _ = rows_of(items[cur[b]])
                j = a0 + r - int(start)
                t[b] = f(tab.coef[min(max(j, a0), e0 - 1), 0])
                if a0 <= j < e0:
                    act[b] = (tab, j)
        x0 = np.asarray(x0_fn(xe, t)).astype(f)
        for b in range(B):
            if cur[b] >= 0 and holds[b][cur[b]] is not None:
                x0[b] = hold_x0(x0[b:b + 1], (holds[b][cur[b]][0][None], holds[b][cur[b]][1][None]))[0]
        for b in range(B):
            if act[b] is None:
                continue
            tab, j = act[b]
            _item_step(state, b, x0, tab, j, hist2[b], corr, own[b][cur[b]], noise_fn, (b, cur[b], j), f"slot {b}")
            _, e0, rid = rows_of(timeline[b][cur[b]])
            if j == tab.steps - 1:
                results[b][cur[b]] = xe[b].copy()
            elif j == e0 - 1:      # the end of a piece that is not the last: what a suspend copies out
                saved[rid] = (e0, [a[b].copy() for a in state])
        if trace is not None:
            trace.append(xe.copy())
    return results


class TablePool:
    """Which solver table lives in which rows of the engine's ``capacity``-row coefficient table during a slot loop.  Pure host
    bookkeeping: ``acquire(key, coef)`` returns ``(row0, write)`` -- the table's first row and whether its rows must be written to the
    engine (``Engine.write_sampler_rows``) -- and counts a user; ``release(key)`` drops one.  Tables are deduplicated by CONTENT (the
    float32 bytes of the rows: two keys with equal rows share them).  A table nobody uses stays resident until room is needed; when an
    acquisition does not fit, the unused tables are dropped and the free rows reused (first fit).  Live tables never move -- their
    slots hold absolute rows --, so an acquisition that fits in no gap between them is refused with the capacity in the message."""

    def __init__(self, capacity: int = TABLE_ROWS):
        self.capacity = int(capacity)
        self._by_content: Dict[bytes, list] = {}      # content -> [row0, rows, users]
        self._content_of: Dict[object, bytes] = {}

    def _gap(self, rows: int, entries) -> Optional[int]:
        at = 0
        for row0, n, _ in sorted(entries, key=lambda e: e[0]):
            if row0 - at >= rows:
                return at
            at = row0 + n
        return at if self.capacity - at >= rows else None

    def rows_in_use(self) -> int:
        return sum(e[1] for e in self._by_content.values() if e[2] > 0)

    def resident(self) -> int:
        return len(self._by_content)

    def acquire(self, key, coef: np.ndarray):
        coef = np.ascontiguousarray(coef, dtype=np.float32)
        if coef.ndim != 2 or coef.shape[1] != NCOEF or coef.shape[0] < 1:
            raise ValueError(f"a table is (rows >= 1, {NCOEF}) float32, got {coef.shape}")
        content = coef.tobytes()
        e = self._by_content.get(content)
        if e is not None:
            e[2] += 1
            self._content_of[key] = content
            return e[0], False
        rows = coef.shape[0]
        row0 = self._gap(rows, self._by_content.values())
        if row0 is None:          # repack: forget the tables no live slot uses
            live = {c: v for c, v in self._by_content.items() if v[2] > 0}
            row0 = self._gap(rows, live.values())
            if row0 is None:
                raise ValueError(f"a table of {rows} rows does not fit: {self.rows_in_use()} of the engine's {self.capacity} table rows are held by "
                                 f"running requests (capacity {self.capacity})")
            self._by_content = live
            self._content_of = {k: c for k, c in self._content_of.items() if c in live}
        self._by_content[content] = [row0, rows, 1]
        self._content_of[key] = content
        return row0, True

    def release(self, key) -> None:
        e = self._by_content.get(self._content_of.get(key, b""))
        if e is None or e[2] <= 0:
            raise ValueError(f"table {key!r} is not in use")
        e[2] -= 1


def plan_slots(steps: Sequence[int], n_slots: int, arrivals: Optional[Sequence[int]] = None):
    """The scheduling of a slot loop as a pure function.  ``steps[i]`` = evaluations of request i (queue order), ``arrivals[i]`` = the loop
    step from which it may start (default 0: all queued at once; non-decreasing).  Greedy and work-conserving: whenever a slot is free and
    a request has arrived, the lowest free slot takes the next request of the queue at once.  Returns a list of events
    ``(loop_step, take, admit)`` in loop order -- ``take`` = [(slot, request)] finished at that step, taken first; ``admit`` =
    [(slot, request)] started at that step -- the loop steps ``run`` between two events being the difference of their loop steps, and the
    loop's length as the last event's step.  No slot idles while a request that has arrived waits, so every request's start is the
    earliest any schedule that keeps the queue order can give it, and the length is at most sum(steps) / n_slots + max(steps)."""
    steps = [int(s) for s in steps]
    if n_slots < 1 or any(s < 1 for s in steps):
        raise ValueError("plan_slots needs n_slots >= 1 and steps >= 1")
    arr = [0] * len(steps) if arrivals is None else [int(a) for a in arrivals]
    if len(arr) != len(steps) or any(a < 0 for a in arr) or any(arr[i] > arr[i + 1] for i in range(len(arr) - 1)):
        raise ValueError("arrivals must hold one non-decreasing loop step >= 0 per request")
    free_at = [0] * n_slots           # loop step at which the slot's item finishes
    holder = [None] * n_slots
    events, nxt, r = [], 0, 0
    while nxt < len(steps) or any(h is not None for h in holder):
        take = [(b, holder[b]) for b in range(n_slots) if holder[b] is not None and free_at[b] <= r]
        for b, _ in take:
            holder[b] = None
        admit = []
        for b in range(n_slots):
            if holder[b] is None and nxt < len(steps) and arr[nxt] <= r:
                holder[b], free_at[b] = nxt, r + steps[nxt]
                admit.append((b, nxt))
                nxt += 1
        if take or admit:
            events.append((r, take, admit))
        nexts = [free_at[b] for b in range(n_slots) if holder[b] is not None]
        if nxt < len(steps) and any(h is None for h in holder):
            nexts.append(arr[nxt])
        if not nexts:
            break
        r = min(nexts)          # (> r: what finished by r was taken, what had arrived by r and found a slot was admitted)
    return events


def plan_slots_preemptive(steps: Sequence[int], n_slots: int, arrivals: Optional[Sequence[int]] = None, priorities: Optional[Sequence[int]] = None):
    """``plan_slots`` for a loop whose running requests can be suspended and resumed, as a pure function.  ``priorities[i]``:
    an int per request, higher = more urgent (default: all 0).  Returns events ``(loop_step, take, suspend, admit)`` in loop order: ``take`` =
    [(slot, request)] finished at that step; ``suspend`` = [(slot, request, done)] -- the request leaves the slot with ``done`` of its rows
    run --; ``admit`` = [(slot, request, done)], ``done`` = 0 an admission and ``done`` > 0 the resume of a suspended request at that row.
    The policy at an event step: (1) take what has finished; (2) fill the free slots, lowest first, from the requests that have arrived and
    wait, the suspended ones among them -- the higher priority first, then queue order; (3) while the best waiting request has a strictly
    higher priority than some running one, suspend the running request of lowest priority -- among equals the one with most rows left, then the
    highest slot --, never one placed at this same step, and give its slot to the waiting request.  Event steps are the steps at which a
    request finishes or arrives.  With equal or no priorities nothing is ever suspended, and the ``(loop_step, take, admit)`` parts are
    ``plan_slots``' events (with ``done`` = 0 added to every admission)."""
    steps = [int(s) for s in steps]
    n = len(steps)
    if n_slots < 1 or any(s < 1 for s in steps):
        raise ValueError("plan_slots_preemptive needs n_slots >= 1 and steps >= 1")
    arr = [0] * n if arrivals is None else [int(a) for a in arrivals]
    if len(arr) != n or any(a < 0 for a in arr) or any(arr[i] > arr[i + 1] for i in range(n - 1)):
        raise ValueError("arrivals must hold one non-decreasing loop step >= 0 per request")
    pri = [0] * n if priorities is None else [int(p) for p in priorities]
    if len(pri) != n:
        raise ValueError("priorities must hold one int per request")
    done = [0] * n
    holder = [None] * n_slots
    since = [0] * n_slots             # loop step at which the slot's request was placed
    finished = [False] * n
    events, r = [], 0

    def rows_run(b):
        return done[holder[b]] + r - since[b]

    while not all(finished):
        take = []
        for b in range(n_slots):
            i = holder[b]
            if i is not None and rows_run(b) >= steps[i]:
                take.append((b, i))
                holder[b], finished[i], done[i] = None, True, steps[i]
        running = {h for h in holder if h is not None}
        waiting = sorted((i for i in range(n) if not finished[i] and i not in running and arr[i] <= r), key=lambda i: (-pri[i], i))
        admit, suspend, placed = [], [], set()
        for b in range(n_slots):
            if holder[b] is None and waiting:
                i = waiting.pop(0)
                holder[b], since[b] = i, r
                admit.append((b, i, done[i]))
                placed.add(b)
        while waiting:
            i = waiting[0]
            victims = [b for b in range(n_slots) if b not in placed and holder[b] is not None and pri[holder[b]] < pri[i]]
            if not victims:
                break
            b = min(victims, key=lambda v: (pri[holder[v]], -(steps[holder[v]] - rows_run(v)), -v))
            j = holder[b]
            done[j] = rows_run(b)
            suspend.append((b, j, done[j]))
            waiting.pop(0)
            holder[b], since[b] = i, r
            admit.append((b, i, done[i]))
            placed.add(b)
            waiting = sorted(waiting + [j], key=lambda q: (-pri[q], q))
        if take or admit or suspend:
            events.append((r, take, suspend, admit))
        nexts = [since[b] + steps[holder[b]] - done[holder[b]] for b in range(n_slots) if holder[b] is not None]
        nexts += [arr[i] for i in range(n) if arr[i] > r]
        if not nexts:
            break
        r = min(nexts)
    return events


def plan_chains(chains: Sequence[Sequence[int]], n_slots: int):
    """The scheduling of a slot loop that serves CHAINED requests, as a pure function.  ``chains[u]`` = the evaluation counts of
    utterance u's chunks in order; chunk (u, j + 1) holds latent frames of chunk (u, j) and so becomes ready when (u, j) has finished.
    Returns events ``(loop_step, take, admit)`` in ``plan_slots``'s format with request ids ``(u, j)``.  Greedy and work-conserving: at every
    event step, after the takes, the ready requests go to the lowest free slots -- first the successors of finished chunks, in utterance
    order (a started utterance finishes first, which bounds the latents kept for later chunks), then first chunks in queue order.  A take
    frees the slot its successor needs, so a successor never waits.  With every chain of length 1 the events are those of
    ``plan_slots([c[0] for c in chains], n_slots)`` with (u, 0) for u."""
    chains = [[int(s) for s in c] for c in chains]
    if n_slots < 1 or any(len(c) < 1 for c in chains) or any(s < 1 for c in chains for s in c):
        raise ValueError("plan_chains needs n_slots >= 1, at least one chunk per chain and steps >= 1")
    free_at = [0] * n_slots
    holder = [None] * n_slots
    events, nxt, r = [], 0, 0
    waiting: List[Tuple[int, int]] = []          # successors that are ready and not admitted yet
    while nxt < len(chains) or waiting or any(h is not None for h in holder):
        take = [(b, holder[b]) for b in range(n_slots) if holder[b] is not None and free_at[b] <= r]
        for b, (u, j) in take:
            holder[b] = None
            if j + 1 < len(chains[u]):
                waiting.append((u, j + 1))
        waiting.sort()
        admit = []
        for b in range(n_slots):
            if holder[b] is not None:
                continue
            if waiting:
                req = waiting.pop(0)
            elif nxt < len(chains):
                req = (nxt, 0)
                nxt += 1
            else:
                break
            holder[b], free_at[b] = req, r + chains[req[0]][req[1]]
            admit.append((b, req))
        if take or admit:
            events.append((r, take, admit))
        nexts = [free_at[b] for b in range(n_slots) if holder[b] is not None]
        if not nexts:
            break
        r = min(nexts)
    return events
