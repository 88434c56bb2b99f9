"""vplines-slam_amd: MI355X-native sliding-window bundle adjustment (and line
front-end) of VPLines-SLAM behind a C ABI (include/vplines_ba.h).

Python here is plumbing only: ctypes bindings to the HIP shared library, the
synthetic workload generator and torch.distributed sharding of window batches.
The HIP library is mandatory -- nothing in this package falls back to a CPU
implementation."""
from . import _build  # noqa: F401
from .capi import (  # noqa: F401
    BaOptions, Preintegration, Prior, Window, SolveReport, Context, SlideTracks, default_options, load_hip_library,
    Session, Frame, ImuFrame, OdoResult, OdoImuOut, OdoDecision, OdoKeyframeRule, FailureLimits,
    default_keyframe_rule, default_failure_limits, failure_detection, InitInput, InitResult,
    SfmInput, SfmResult, sfm_debug_plan, RelPoseInput, RelPoseResult, relpose_debug_plan,
    SelectParams, SelectInput, SelectResult, SelectFrame, OdoSelectResult, select_debug_book,
    LoopInput, LoopOptions, LoopResult, default_loop_options, loop_debug_plan,
    PoseGraphInput, PoseGraphResult, PgOptions, default_pg_options,
    PoseGraphSession, PgsOptions, default_pgs_options,
    GlobalFusionInput, GlobalFusionResult, GfOptions, default_gf_options, gf_debug_plan, local_cartesian,
    GlobalFusionSession,
    MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_NONE, PRIOR_PIVOTED_CHOLESKY, PRIOR_EIGEN,
)
from . import workload  # noqa: F401
from . import shard  # noqa: F401
from . import frontend  # noqa: F401
from .frontend import TrackerSession, TrackerOptions, TrackerResult, default_tracker_options  # noqa: F401
from .frontend import PointCamera, PointTrackerSession, PointTrackerOptions, PointTrackerResult, default_point_tracker_options  # noqa: F401
from .frontend import LoopDetector, LoopDetectorOptions, LoopDetectorResult, Vocabulary, default_loop_detector_options  # noqa: F401
