"""The reference's 3DIdent data pipeline (datasets/threedident_dataset.py) on the GPU: latent lookup and image batches."""
from .image_table import ImageTable
from .threedident_dataset import (BatchLoader, IndexFlatL2, SequentialThreeDIdentDataset, ThreeDIdentDataset,
                                  ThreeDIdentLatentPairs)

__all__ = ["IndexFlatL2", "ThreeDIdentLatentPairs", "ImageTable", "ThreeDIdentDataset", "SequentialThreeDIdentDataset", "BatchLoader"]
