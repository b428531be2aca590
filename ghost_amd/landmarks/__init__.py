"""The 106-point face landmark model (insightface 2d106det) on the MI355X."""
from .handler import (Handler, identity_landmarks, identity_masks, identity_masks_device, present_runs,
                      run_indices)
from .net import Landmark106
from .pack import param_specs

__all__ = ["Handler", "Landmark106", "identity_landmarks", "identity_masks", "identity_masks_device", "param_specs",
           "present_runs", "run_indices"]
