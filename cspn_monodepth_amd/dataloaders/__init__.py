"""The device side of the reference's `dataloaders` package: what its loader does per frame on the host, for batches that already
sit on the GPU (nyu_dataloader.nyu_dataloader: the train / val transforms on raw frames; nyu_dataloader.dense_to_sparse)."""
from . import nyu_dataloader

__all__ = ["nyu_dataloader"]
