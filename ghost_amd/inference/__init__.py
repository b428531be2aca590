"""Drop-ins for the swap-batch boundary of utils/inference (faceshifter_run.py, core.py)."""
from .align import (align_crops, crop_face, crop_frames_and_get_transforms, estimate_norm,  # noqa: F401
                    similarity_transform, smooth_landmarks)
from .core import swap_identity_frames, transform_target_to_torch  # noqa: F401
from .faceshifter_run import faceshifter_batch, faceshifter_batch_u8  # noqa: F401
from .graphed import GraphedSwap  # noqa: F401
from .roi import (align_crops_roi, blend_swaps_roi, crop_frames_and_get_transforms_roi, download_rois,  # noqa: F401
                  face_rois, plan_rois, upload_rois)
from .roi_pack import RoiStaging, download_rois_packed, packed_layout, upload_rois_packed  # noqa: F401
