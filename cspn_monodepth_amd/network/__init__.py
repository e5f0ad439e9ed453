"""Pieces of the reference's network/ package that sit on the hot path's doorstep."""
from . import conv_tuning, inplace_abn, up_pooling
from .conv_tuning import use_tuned_conv_db
from .inplace_abn import ABN, InPlaceABN, InPlaceABNSync, InPlaceABNSyncWrapper, InPlaceABNWrapper, convert_batchnorm
from .up_pooling import MyBlock

__all__ = ["conv_tuning", "up_pooling", "inplace_abn", "MyBlock", "use_tuned_conv_db", "unet_ours", "unet_cspn_nyu",
           "ABN", "InPlaceABN", "InPlaceABNSync", "InPlaceABNWrapper", "InPlaceABNSyncWrapper", "convert_batchnorm"]

_LAZY = ("unet_ours", "unet_cspn_nyu")      # the host models: imported on first use, importing the package stays cheap


def __getattr__(name):
    if name in _LAZY:
        import importlib
        return importlib.import_module("." + name, __name__)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
