"""The 106-point face landmark model (insightface 2d106det) on the MI355X."""
from .handler import Handler, identity_landmarks, identity_masks, present_runs
from .net import Landmark106
from .pack import param_specs

__all__ = ["Handler", "Landmark106", "identity_landmarks", "identity_masks", "param_specs", "present_runs"]
