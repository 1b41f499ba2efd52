"""orbslamm_amd -- MI355X-native ORB front-end (extract + Hamming match) for ORBSLAMM.

Only what the hot path needs: csrc/ (HIP kernels + C ABI), and thin ctypes mirrors
of the reference's ORBextractor / ORBmatcher interfaces."""
from .extractor import ORBextractor, unpack_candidates  # noqa: F401
from .matcher import ORBmatcher, make_grid  # noqa: F401
from .vocabulary import ORBVocabulary  # noqa: F401
from .keyframe_db import KeyFrameDatabase, KeyFramePool  # noqa: F401
from .pnp import PnPsolver, make_pnp_sets  # noqa: F401
from .local_mapping import compute_f12, create_new_map_points, fuse_batch, level_breaks  # noqa: F401
from .loop_closing import search_and_fuse, decompose_sim3  # noqa: F401
from .optimizer import pose_optimization, pose_optimization_batch  # noqa: F401
from .optimizer import optimize_sim3, optimize_sim3_batch, sim3_from_rts  # noqa: F401
from .initial_map import initial_map, initial_map_batch  # noqa: F401
from .map_pool import KeyFrameStore, MapPool  # noqa: F401
from .map_pool import REFRESH_DESCRIPTOR, REFRESH_DTYPE, REFRESH_MAX_OBS, REFRESH_NORMAL_DEPTH  # noqa: F401
from .map_pool import CORRECT_KF_DTYPE, CORRECT_POINT_DTYPE  # noqa: F401
from .track_pose import pack_reloc_jobs, relocalize, relocalize_raw, track_pose, track_reference  # noqa: F401
from .track_pose import pack_motion_jobs, track_motion_model, track_motion_model_raw  # noqa: F401
from .compute_sim3 import compute_sim3, compute_sim3_batch  # noqa: F401
from ._lib import KP_DTYPE, OrbError  # noqa: F401
