"""``from sampler.uni_pc import NoiseScheduleVP, model_wrapper, UniPC``: UniPC-bh (multistep, orders 1-3, ``bh1`` | ``bh2``) on this
project's coefficient table and float32 recurrence (``sampler._driver``)."""
from ._driver import NoiseScheduleVP, Solver, model_wrapper

__all__ = ["NoiseScheduleVP", "model_wrapper", "UniPC"]


class UniPC(Solver):
    solver = "unipc"

    def __init__(self, model_fn, noise_schedule, algorithm_type="data_prediction", correcting_x0_fn=None, correcting_xt_fn=None,
                 thresholding_max_val=1., dynamic_thresholding_ratio=0.995, variant="bh1"):
        if algorithm_type != "data_prediction":
            raise ValueError(f"algorithm_type must be 'data_prediction' (the table's recurrence runs on the predicted x0; 'noise_prediction' is not served), got {algorithm_type!r}")
        self.algorithm_type = algorithm_type
        super().__init__(model_fn, noise_schedule, correcting_x0_fn, correcting_xt_fn, thresholding_max_val, dynamic_thresholding_ratio, variant)

    def sample(self, x, steps=20, t_start=None, t_end=None, order=2, skip_type="time_uniform", method="multistep", lower_order_final=True,
               denoise_to_zero=False, atol=0.0078, rtol=0.05, return_intermediate=False):
        """x_T -> the sample in ``x.dtype``.  ``atol`` / ``rtol`` belong to the adaptive method and are unused."""
        return self._sample(x, steps, order, method, return_intermediate,
                            dict(skip_type=skip_type, lower_order_final=lower_order_final, denoise_to_zero=denoise_to_zero, variant=self.variant,
                                 t_start=t_start, t_end=t_end))
