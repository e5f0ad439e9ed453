"""Pieces of the reference's network/ package that sit on the hot path's doorstep."""
from . import conv_tuning, up_pooling
from .conv_tuning import use_tuned_conv_db
from .up_pooling import MyBlock

__all__ = ["conv_tuning", "up_pooling", "MyBlock", "use_tuned_conv_db", "unet_ours", "unet_cspn_nyu"]

_LAZY = ("unet_ours", "unet_cspn_nyu")      # the host models: imported on first use, importing the package stays cheap


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
