"""scream_amd: MI355X-native registration hot path of xujiabo/SCREAM.

Importing the package is cheap and CPU-safe (synthetic data, packing metadata); anything that
computes needs libscream_hip.so and an MI355X and raises ``ScreamHipError`` otherwise.
"""
from ._lib import ScreamHipError  # noqa: F401
from .chamfer import ChamferDistance, chamfer_packed  # noqa: F401
from .dsm import extract_dsm, extract_dsm_batch, make_dsm_dem, make_dsm_dem_batch, tile_windows  # noqa: F401
from .optim import FusedAdam  # noqa: F401
from .overlap import (overlap_batch, prepare_3dmatch_batch, radius_count_batch, radius_pairs_batch,  # noqa: F401
                      select_outputs)
from .prep import (PreparedPairs, packed_l1_loss, prepare_3dmatch_train, prepare_3dmatch_val, prepare_kitti_train,  # noqa: F401
                   prepare_kitti_val, prepare_pairs, sample_perturbations)
from .rawicp import RawIcpRun, icp_raw_batch, raw_nn_batch  # noqa: F401
from .voxel import voxel_down_sample, voxel_down_sample_batch  # noqa: F401

__all__ = ["ScreamHipError", "voxel_down_sample", "voxel_down_sample_batch", "extract_dsm", "extract_dsm_batch", "make_dsm_dem",
           "make_dsm_dem_batch", "tile_windows", "radius_count_batch", "radius_pairs_batch", "overlap_batch", "prepare_3dmatch_batch",
           "select_outputs", "sample_perturbations", "prepare_pairs", "PreparedPairs", "prepare_3dmatch_train", "prepare_3dmatch_val",
           "prepare_kitti_train", "prepare_kitti_val", "packed_l1_loss", "icp_raw_batch", "raw_nn_batch", "RawIcpRun", "FusedAdam",
           "chamfer_packed", "ChamferDistance"]
__version__ = "0.1.0"
