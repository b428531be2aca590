"""The reference's ``--use_sr`` face enhancer on MI355X (inference.py:42-50, 105-106): LIP-SPADE generator,
``Pix2PixModel`` wrapper and ``face_enhancement``."""
from .config_sr import TestOptions
from .enhance import Pix2PixModel, face_enhancement
from .generator import LIPSPADEGenerator

__all__ = ["TestOptions", "LIPSPADEGenerator", "Pix2PixModel", "face_enhancement"]
