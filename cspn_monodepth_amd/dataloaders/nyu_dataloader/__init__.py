"""dataloaders/nyu_dataloader of the reference: the NYU train / val transforms on raw frames (nyu_dataloader), the sparse-depth
sampler and the RGB-D assembly (dense_to_sparse)."""
from . import dense_to_sparse, nyu_dataloader
from .dense_to_sparse import SimulatedStereo, UniformSampling, create_rgbd, create_sparse_depth
from .nyu_dataloader import draw_train_params, train_transform, val_transform

__all__ = ["dense_to_sparse", "nyu_dataloader", "SimulatedStereo", "UniformSampling", "create_rgbd", "create_sparse_depth",
           "draw_train_params", "train_transform", "val_transform"]
