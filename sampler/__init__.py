"""``sampler``: the solver classes the NS2VC code imports (``sampler.dpm_solver``, ``sampler.uni_pc``), as drivers of this project's sampling
loop.  With this repository first on ``PYTHONPATH`` the unmodified ``NaturalSpeech2.sample`` reaches the captured loop of the HIP engine
(DESIGN.md 4.19).

``sampler.capture`` (default True; the environment variable ``NS2VC_SAMPLER_CAPTURE=0`` turns it off): whether a ``sample`` call whose model
is recognised as the drop-in ``unet1d.UNet1DConditionModel`` is handed to ``ns2vc_amd.pipeline.Denoiser.sample``.  False: the model is called
once per step, as the caller's wrapper expects.

Importing this package loads neither ``oracle`` nor ``libns2vc_hip.so``."""
import os

capture = os.environ.get("NS2VC_SAMPLER_CAPTURE", "1") != "0"

__all__ = ["capture", "dpm_solver", "uni_pc"]
