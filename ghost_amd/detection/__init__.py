"""The SCRFD face detector on the device: the network, its letterbox and SCRFD.detect's post-processing."""
from . import pack
from .handler import Face_detect_crop
from .net import SCRFD
from .pack import fold_bn, letterbox_geometry, select_max_num

__all__ = ["SCRFD", "Face_detect_crop", "fold_bn", "letterbox_geometry", "select_max_num", "pack"]
