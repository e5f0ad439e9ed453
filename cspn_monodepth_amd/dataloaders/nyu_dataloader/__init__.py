"""dataloaders/nyu_dataloader of the reference: the sparse-depth sampler and the RGB-D assembly (dense_to_sparse)."""
from . import dense_to_sparse
from .dense_to_sparse import SimulatedStereo, UniformSampling, create_rgbd, create_sparse_depth

__all__ = ["dense_to_sparse", "SimulatedStereo", "UniformSampling", "create_rgbd", "create_sparse_depth"]
