"""``from sampler.dpm_solver import NoiseScheduleVP, model_wrapper, DPM_Solver``: DPM-Solver++ (multistep, orders 1-3) on this project's
coefficient table and float32 recurrence (``sampler._driver``)."""
from ._driver import NoiseScheduleVP, Solver, model_wrapper

__all__ = ["NoiseScheduleVP", "model_wrapper", "DPM_Solver"]


class DPM_Solver(Solver):
    solver = "dpmsolver++"

    def __init__(self, model_fn, noise_schedule, algorithm_type="dpmsolver++", correcting_x0_fn=None, correcting_xt_fn=None,
                 thresholding_max_val=1., dynamic_thresholding_ratio=0.995):
        if algorithm_type != "dpmsolver++":
            raise ValueError(f"algorithm_type must be 'dpmsolver++' (the table's recurrence runs on the predicted x0; the noise-prediction 'dpmsolver' is not served), got {algorithm_type!r}")
        self.algorithm_type = algorithm_type
        super().__init__(model_fn, noise_schedule, correcting_x0_fn, correcting_xt_fn, thresholding_max_val, dynamic_thresholding_ratio)

    def sample(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep", lower_order_final=True,
               denoise_to_zero=False, solver_type="dpmsolver", atol=0.0078, rtol=0.05, return_intermediate=False):
        """x_T -> the sample in ``x.dtype``.  ``atol`` / ``rtol`` belong to the adaptive method and are unused."""
        return self._sample(x, steps, order, method, return_intermediate,
                            dict(skip_type=skip_type, lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, solver_type=solver_type,
                                 t_start=t_start, t_end=t_end))

    def inverse(self, *args, **kwargs):
        raise ValueError("inverse is not served (the table runs from noise to data only)")

    def add_noise(self, *args, **kwargs):
        raise ValueError("add_noise is not served")
