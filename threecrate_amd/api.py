"""Host-side mirror of the reference interface for the normals + ICP path.

Names, argument meaning and error behaviour follow threecrate-algorithms (normals.rs,
registration.rs) and the threecrate-gpu facade (device.rs, normals.rs, icp.rs); call shapes
follow the pyo3 module (threecrate-python/src/lib.rs:827-1010): N x 3 float32 in,
N x 6 / N x 3 normals and 4 x 4 float32 + mse + iterations + converged out.

Every function runs the HIP path through the C ABI (include/threecrate_hip.h).  numpy inputs
take the host entry points (H2D staging inside the library); torch CUDA tensors take the
*_device entry points with zero copies.  There is no CPU fallback.
"""
import ctypes as C
import os
import weakref
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib

IDENTITY = np.array([0, 0, 0, 1, 0, 0, 0], dtype=np.float32)


# ---- threecrate_core::Error (threecrate-core/src/error.rs:7-28) ------------------------------
class Error(Exception):
    pass


class InvalidData(Error):
    pass


class AlgorithmError(Error):
    pass


class GpuError(Error):
    pass


class Unsupported(Error):
    pass


_ERR = {_lib.TC_INVALID_DATA: InvalidData, _lib.TC_ALGORITHM: AlgorithmError, _lib.TC_GPU: GpuError,
        _lib.TC_UNSUPPORTED: Unsupported}


@dataclass
class NormalEstimationConfig:
    """normals.rs:17-37"""
    k_neighbors: int = 10
    radius: Optional[float] = None
    consistent_orientation: bool = True
    viewpoint: Optional[tuple] = None


@dataclass
class IcpScaleLevel:
    """registration.rs:27-35"""
    voxel_size: float
    max_iterations: int
    max_correspondence_distance: Optional[float] = None


@dataclass
class MultiScaleIcpConfig:
    """registration.rs:38-71 (same defaults)"""
    levels: list = field(default_factory=lambda: [IcpScaleLevel(0.20, 10, 0.50), IcpScaleLevel(0.10, 10, 0.25),
                                                  IcpScaleLevel(0.05, 15, 0.15)])
    final_refinement_iterations: int = 10
    final_max_correspondence_distance: Optional[float] = 0.10
    convergence_threshold: float = 1e-5


@dataclass
class GicpConfig:
    """gicp.rs:25-40"""
    max_iterations: int = 50
    max_correspondence_distance: float = 1.0
    convergence_threshold: float = 1e-6
    k_correspondences: int = 20


@dataclass
class KissIcpConfig:
    """kiss_icp.rs:28-49"""
    voxel_size: float = 1.0
    max_range: float = 100.0
    min_range: float = 0.5
    max_iterations: int = 50


@dataclass
class OutlierResult:
    """What an outlier filter leaves (filtering.rs:167-395): the kept points in input order, their original indices, and for the
    statistical filter every input point's mean distance and the threshold the means were compared with."""
    points: object
    index: object
    mean_distance: object = None
    threshold: float = None


@dataclass
class PlaneSegmentationResult:
    """What segment_plane returns (segmentation.rs:94-103; the wheel's PlaneSegmentationResult, threecrate-python/src/lib.rs:636-690):
    the (4,) float32 coefficients a, b, c, d of a*x + b*y + c*z + d = 0, the inliers' original indices in ascending order (uint32;
    int32 on the device; None when no list was asked for), and the number of RANSAC iterations, which is the max_iters given.
    best_iteration (the winning iteration) and num_inliers are this backend's additions."""
    plane_coefficients: object
    inlier_indices: object
    iterations: int
    best_iteration: int = 0
    num_inliers: int = 0


@dataclass
class GpuPlaneSegmentationConfig:
    """threecrate-gpu/src/segmentation.rs:194-213"""
    max_iterations: int = 1000
    distance_threshold: float = 0.02
    min_inliers: int = 1


@dataclass
class NdtConfig:
    """ndt_registration.rs:15-38 (same defaults)"""
    resolution: float = 1.0
    step_size: float = 0.1
    max_iterations: int = 35
    epsilon: float = 1e-4
    min_points_per_voxel: int = 5


@dataclass
class NdtResult:
    """ndt_registration.rs:42-51; `transformation` is the 7-float Isometry3 (qi qj qk qw tx ty tz).  `score` belongs to the last pose
    that was evaluated.  n_voxels (voxels of the target's map) and n_hits (source points of the last evaluation that fell into
    one) are this backend's additions."""
    transformation: np.ndarray
    score: float
    iterations: int
    converged: bool
    n_voxels: int = 0
    n_hits: int = 0

    @property
    def matrix(self):
        """4 x 4 float32 homogeneous matrix (threecrate-python/src/lib.rs:48-61)."""
        return isometry_to_matrix(self.transformation)


@dataclass
class RansacResult:
    """What ransac_correspondences returns (include/threecrate_hip_global.h): the winner's stored transform as 12 float32 (R row-major,
    then t; the identity when nothing won), its score, score / m, the iterations the sequential loop would have run, the winning
    iteration, whether the early-exit count was reached; with candidates=True every candidate's transform (n, 12) and score (n,)."""
    transform: np.ndarray
    inlier_count: int
    inlier_ratio: float
    iterations_run: int
    best_iteration: int
    early_exit: bool
    cand_transform: object = None
    cand_count: object = None

    @property
    def matrix(self):
        """4 x 4 float32 homogeneous matrix: the stored bits"""
        m = np.eye(4, dtype=np.float32)
        m[:3, :3], m[:3, 3] = self.transform[:9].reshape(3, 3), self.transform[9:]
        return m


@dataclass
class GlobalRegistrationConfig:
    """global_registration.rs:27-62 (same fields, same defaults).  seed is this backend's addition: it is XORed into the initial state
    of the RANSAC sample generator (the reference draws from the thread's RNG and cannot be reproduced)."""
    ransac_iterations: int = 50_000
    distance_threshold: float = 0.05
    inlier_ratio: float = 0.25
    fpfh_radius: float = 0.25
    fpfh_k_neighbors: int = 10
    normal_k_neighbors: int = 10
    refine_with_icp: bool = True
    icp_max_iterations: int = 50
    icp_distance_threshold: Optional[float] = None
    seed: int = 0


@dataclass
class GlobalRegistrationResult:
    """global_registration.rs:70-79: `transformation` is the 7-float Isometry3 (qi qj qk qw tx ty tz) of the refinement when there is
    one, else RANSAC's rotation as a quaternion; inlier_count / inlier_ratio are RANSAC's; icp_result is the refinement's ICPResult or
    None.  `ransac` (the RansacResult, with the stored matrix bits) is this backend's addition."""
    transformation: np.ndarray
    inlier_count: int
    inlier_ratio: float
    icp_result: object = None
    ransac: object = None

    @property
    def matrix(self):
        """4 x 4 float32: the refinement's, else RANSAC's stored matrix"""
        return self.icp_result.matrix if self.icp_result is not None else self.ransac.matrix


@dataclass
class CameraIntrinsics:
    """CameraIntrinsics (threecrate-gpu/src/tsdf.rs:41-50).  depth_scale is kept for the reference's call shape and, as in its shader,
    never read: depth images are in metres."""
    fx: float
    fy: float
    cx: float
    cy: float
    width: int
    height: int
    depth_scale: float = 1.0


@dataclass
class ICPResult:
    """registration.rs:13-24; `transformation` is the 7-float Isometry3 (qi qj qk qw tx ty tz)."""
    transformation: np.ndarray
    mse: float
    iterations: int
    converged: bool
    correspondences: np.ndarray = field(default_factory=lambda: np.zeros((0, 2), np.int64))
    corr_target: object = None   # dense per-source target index (0xFFFFFFFF = none), numpy or torch

    @property
    def matrix(self):
        """4 x 4 float32 homogeneous matrix (threecrate-python/src/lib.rs:48-61)."""
        return isometry_to_matrix(self.transformation)


def isometry_to_matrix(T):
    x, y, z, w = [np.float32(v) for v in T[:4]]
    two = np.float32(2)
    ww, xx, yy, zz = w * w, x * x, y * y, z * z
    m = np.eye(4, dtype=np.float32)
    m[0, 0] = ww + xx - yy - zz; m[0, 1] = x * y * two - w * z * two; m[0, 2] = w * y * two + x * z * two
    m[1, 0] = w * z * two + x * y * two; m[1, 1] = ww - xx + yy - zz; m[1, 2] = y * z * two - w * x * two
    m[2, 0] = x * z * two - w * y * two; m[2, 1] = w * x * two + y * z * two; m[2, 2] = ww - xx - yy + zz
    m[:3, 3] = T[4:7]
    return m


def rotation_to_isometry(transform12):
    """12 floats (R row-major, t) -> the 7-float Isometry3 (qi qj qk qw tx ty tz), in numpy f64 (Shepperd's branches, as
    UnitQuaternion::from_rotation_matrix), rounded once"""
    T = np.asarray(transform12, np.float64).reshape(12)
    r = T[:9].reshape(3, 3)
    tr = r[0, 0] + r[1, 1] + r[2, 2]
    if tr > 0.0:
        d = np.sqrt(tr + 1.0) * 2.0
        w, i, j, k = 0.25 * d, (r[2, 1] - r[1, 2]) / d, (r[0, 2] - r[2, 0]) / d, (r[1, 0] - r[0, 1]) / d
    elif r[0, 0] > r[1, 1] and r[0, 0] > r[2, 2]:
        d = np.sqrt(1.0 + r[0, 0] - r[1, 1] - r[2, 2]) * 2.0
        w, i, j, k = (r[2, 1] - r[1, 2]) / d, 0.25 * d, (r[0, 1] + r[1, 0]) / d, (r[0, 2] + r[2, 0]) / d
    elif r[1, 1] > r[2, 2]:
        d = np.sqrt(1.0 + r[1, 1] - r[0, 0] - r[2, 2]) * 2.0
        w, i, j, k = (r[0, 2] - r[2, 0]) / d, (r[0, 1] + r[1, 0]) / d, 0.25 * d, (r[1, 2] + r[2, 1]) / d
    else:
        d = np.sqrt(1.0 + r[2, 2] - r[0, 0] - r[1, 1]) * 2.0
        w, i, j, k = (r[1, 0] - r[0, 1]) / d, (r[0, 2] + r[2, 0]) / d, (r[1, 2] + r[2, 1]) / d, 0.25 * d
    q = np.array([i, j, k, w])
    q /= np.linalg.norm(q)
    return np.concatenate([q, T[9:]]).astype(np.float32)


_NO_VOXELS = np.zeros(1, np.float32)      # what marching_cubes passes as `values` for a grid of zero voxels


def _is_torch(x):
    return type(x).__module__.startswith("torch")


# ---- array adapters: the one place an input is converted, an output allocated, a correspondence buffer cut ------------
def _f32(a, on_device=None):
    """float32 and contiguous, in place where the input already is.  on_device None: a torch tensor stays a torch tensor, anything
    else -> numpy.  True / False: the road is already chosen (by the call's first array, or because the entry point exists on
    one side only) and `a` is converted for THAT road: a host array has no .detach(), np.asarray refuses a device tensor, so an
    argument of the other kind raises here and never reaches the library as a pointer into the wrong memory."""
    if _is_torch(a) if on_device is None else on_device:
        import torch
        return a.detach().to(torch.float32).contiguous()
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32))


def _as_host(a, cols=3):
    a = _f32(a, False)
    if a.size == 0:
        return a.reshape(0, cols)
    return a.reshape(-1, cols)


def _ptr(x):
    return x.data_ptr() if _is_torch(x) else x.ctypes.data


class _points:
    """_points(a, cols=3): an (n, cols) float32 input as an entry point takes it.  `a` keeps the converted array alive, `ptr` / `n`
    go to the library, `device` is the tensor's device (None for host input, which takes the host entry point: is_torch picks
    the road)."""
    __slots__ = ("a", "ptr", "n", "device")

    def __init__(self, a, cols=3, on_device=None):
        if _is_torch(a) if on_device is None else on_device:
            self.a = _f32(a, True).reshape(-1, cols)
            self.device = self.a.device
        else:
            self.a, self.device = _as_host(a, cols), None
        self.ptr, self.n = _ptr(self.a), self.a.shape[0]

    @property
    def is_torch(self):
        return self.device is not None


class _road_of:
    """the road an array that is no float cloud picks (an index array alone: the faces of mesh_adjacency): what _u32, _new and
    GpuContext._road read of a _points"""
    __slots__ = ("device",)

    def __init__(self, a):
        self.device = a.device if _is_torch(a) else None

    @property
    def is_torch(self):
        return self.device is not None


def _normals_arg(normals, on_device=None):
    """(N, 3) Vector3f, flat, or the (N, 6) NormalPoint3f array of estimate_normals, whose normal columns are read in place
    (stride 6, 12 bytes in) -> (pointer, count, stride, the array that owns the memory)."""
    n = _f32(normals, on_device)
    stride = 6 if (n.ndim == 2 and n.shape[1] == 6) else 3
    count = n.shape[0] if n.ndim == 2 else (n.numel() if _is_torch(n) else n.size) // 3
    return _ptr(n) + (12 if stride == 6 else 0), count, stride, n


def _u32(a, like, cols=None):
    """an index array for the road `like` (a _points) chose: uint32 on the host, the same bits as int32 on like's device.  A host array
    given with device clouds is moved there; a wider integer is reduced mod 2^32 (0xFFFFFFFF stays the out-of-range marker it is)"""
    if like.is_torch:
        import torch
        if not _is_torch(a):
            a = torch.from_numpy((np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))
        elif a.dtype != torch.int32:
            a = a.detach().to(torch.int64) & 0xFFFFFFFF
            a = torch.where(a >= (1 << 31), a - (1 << 32), a)           # the same 32 bits as a signed value: the narrowing is exact
        a = a.detach().to(device=like.device, dtype=torch.int32).contiguous()
    else:
        if _is_torch(a):
            a = a.detach().cpu().numpy()
        a = np.ascontiguousarray((np.asarray(a).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32))
    return a.reshape(-1) if cols is None else a.reshape(-1, cols)


def _init7(init):
    """the 7-float start pose (qi qj qk qw tx ty tz), identity by default"""
    return np.ascontiguousarray(IDENTITY if init is None else np.asarray(init, np.float32).reshape(7))


_DEVICE_DTYPE = {np.float32: "float32", np.uint32: "int32", np.int32: "int32", np.uint64: "int64", np.uint8: "uint8"}     # torch has no unsigned 32 / 64: same bits


def _new(device, shape, dtype=np.float32, zeros=False):
    """an output buffer next to its input: a torch tensor on `device`, numpy for None"""
    if device is None:
        return (np.zeros if zeros else np.empty)(shape, dtype)
    import torch
    return (torch.zeros if zeros else torch.empty)(shape, dtype=getattr(torch, _DEVICE_DTYPE[dtype]), device=device)


def _search_out(device, nq, k):
    """idx | dist | count of a k-NN / radius query over nq queries, zeroed (entries past count[q] are never written)"""
    kk = max(int(k), 1)
    return _new(device, (nq, kk), np.uint32, True), _new(device, (nq, kk), zeros=True), _new(device, nq, np.uint32, True)


def _first_row(idx, dist, cnt):
    """the [(index, distance), ...] of a one-query batch"""
    return [(int(idx[0, i]), float(dist[0, i])) for i in range(int(cnt[0]))]


def _one_query(query):
    return np.asarray(query, np.float32).reshape(1, 3)


def _corr_buffer(r, device, ns):
    """the dense per-source target index an ICP entry point fills through r.corr_target (never empty: the library wants a pointer)"""
    corr = _new(device, max(1, ns), np.uint32)
    r.corr_target = _ptr(corr)
    return corr


def _cut_corr(corr, n, want, device_bits=True):
    """What the caller sees of that buffer: its first n entries.  A device buffer is widened to int64 and masked (0xFFFFFFFF =
    none, as in the host buffer) unless correspondences="device" asked for it as written (int32 bits, -1 = none)."""
    if corr is None:
        return None
    corr = corr[:n]
    if _is_torch(corr) and not (device_bits and want == "device"):
        import torch
        corr = corr.to(torch.int64) & 0xFFFFFFFF
    return corr


class _Handle:
    """Lifetime of a library handle `_h` (destroyed through `_L`): close() destroys it once, a dropped object closes itself and
    keeps quiet about it (interpreter shutdown, a constructor that raised before there was a handle)."""
    _destroy = None         # the tc_*_destroy export

    def close(self):
        if getattr(self, "_h", None):
            getattr(self._L, self._destroy)(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GpuContext(_Handle):
    """GpuContext::new (threecrate-gpu/src/device.rs:16-50): one HIP device + one stream."""
    _destroy = "tc_context_destroy"

    def __init__(self, device: int = 0, stream=None):
        self._L = _lib.load()
        h = C.c_void_p()
        if stream is None:
            rc = self._L.tc_context_create(device, C.byref(h))
        else:
            rc = self._L.tc_context_create_on_stream(device, C.c_void_p(stream), C.byref(h))
        if rc != _lib.TC_OK:
            raise GpuError(f"no usable HIP device {device} (tc_status {rc}); threecrate_amd has no CPU fallback")
        self._h = h
        self.device = device
        self.stream = stream          # raw hipStream_t the context enqueues on (None: its own stream)

    def _track(self, child):
        """A handle made on this context (a cloud, a search index, a frame stream, a TSDF volume, a voxel map) points into it: the
        context remembers its live children (weakly) and close() destroys them before itself, so no handle is ever destroyed, by
        hand or by a late __del__, after the context it points into."""
        if not hasattr(self, "_children"):
            self._children = weakref.WeakSet()
        self._children.add(child)
        return self

    def close(self):
        for child in list(getattr(self, "_children", ())):
            child.close()
        super().close()

    def trim(self):
        """tc_context_trim: release the device memory parked by destroyed handles (the context keeps a few handles' worth for
        reuse) -- before handing the GPU to another allocator"""
        self._check(self._L.tc_context_trim(self._h))

    def _check(self, rc):
        if rc != _lib.TC_OK:
            msg = self._L.tc_last_error_message(self._h).decode()
            raise _ERR.get(rc, Error)(msg)

    def _order(self, device):
        """Stream ordering rule of the *_device entry points (include/threecrate_hip.h): the library reads the
        tensors on the context's stream, torch produced them (conversions, slices, the caller's own ops) on its
        current stream -> make the context's stream wait for torch's (an event, no host wait)."""
        import torch
        cur = torch.cuda.current_stream(device).cuda_stream
        if self.stream is None or self.stream != cur:
            self._check(self._L.tc_context_wait_stream(self._h, C.c_void_p(cur)))

    def _release(self, device):
        """the reverse of _order: torch's current stream waits for what the context's stream holds now (a buffer torch owns
        was handed to a stream-ordered entry point and may be overwritten or freed by torch next)"""
        import torch
        cur = torch.cuda.current_stream(device).cuda_stream
        if self.stream is None or self.stream != cur:
            self._check(self._L.tc_stream_wait_context(self._h, C.c_void_p(cur)))

    def _road(self, x, host_fn, device_fn):
        """the entry point for x's kind; the device one reads x on the context's stream, which is ordered behind torch's first"""
        if x.is_torch:
            self._order(x.device)
            return device_fn
        return host_fn

    @staticmethod
    def _max_dist(d):
        """Option<f32> -> the ABI's encoding (< 0 = None).  A negative Some(d) must not alias None (see _reject_all):
        it is returned as None."""
        if d is None:
            return -1.0
        return None if float(d) < 0.0 else float(d)

    @staticmethod
    def _max_dist_as_given(d):
        """The same encoding where there is no _reject_all road (FrameStream's config, the multiscale levels), with one difference:
        a negative Some(d) goes to the library as it is, and reads as None there."""
        return -1.0 if d is None else float(d)

    @staticmethod
    def _reject_all(ns, nt, max_iters, normals_len=None):
        """A negative Some(max_correspondence_distance): the reference rejects every pair (registration.rs:100-101,
        `distance > d` always holds), i.e. after its validation (:266-276 / :517-531) the first iteration fails with
        "Insufficient correspondences" (:311-315 / :568-572)."""
        if ns == 0 or nt == 0:
            raise InvalidData("Source or target point cloud is empty")
        if normals_len is not None and normals_len != nt:
            raise InvalidData("target_normals length must equal the number of target points")
        if max_iters == 0:
            raise InvalidData("Max iterations must be positive")
        raise AlgorithmError("Insufficient correspondences found (negative max_correspondence_distance rejects every pair)")

    # ---- profiling ----
    def profile_enable(self, on=True):
        """False/0 off, True/1 every kernel, 2 = sampled events on the dominant kernel only, 3 = no events: the ICP main pass
        counts its searches instead (search_stats())."""
        self._L.tc_profile_enable(self._h, int(on))

    def profile_reset(self):
        self._L.tc_profile_reset(self._h)

    def debug_counter(self, which="indexed_points"):
        """work counters since the context was created (tc_debug_counter): "indexed_points" = points that went through an index
        build, "index_builds" = the builds"""
        return int(self._L.tc_debug_counter(self._h, {"indexed_points": _lib.TC_COUNTER_INDEXED_POINTS, "index_builds": _lib.TC_COUNTER_INDEX_BUILDS}[which]))

    def search_stats(self):
        """Search statistics of the ICP main pass over the registrations run since profile_enable(3) (SURVEY 8d's secondary
        figures; tc_debug_counter TC_COUNTER_ICP_*): raw counters + the derived per-search / lock-step figures.  A candidate step
        = four consecutive target records = four distance evaluations of one lane."""
        c = {k: int(self._L.tc_debug_counter(self._h, v)) for k, v in (
            ("iterations", _lib.TC_COUNTER_ICP_ITERATIONS), ("wave_trips", _lib.TC_COUNTER_ICP_TRIPS),
            ("wave_trips_without_a_search", _lib.TC_COUNTER_ICP_TRIPS_WITHOUT_SEARCH), ("searches", _lib.TC_COUNTER_ICP_SEARCHES),
            ("candidate_steps_needed", _lib.TC_COUNTER_ICP_STEPS_NEEDED), ("candidate_steps_taken_by_slowest_lanes", _lib.TC_COUNTER_ICP_STEPS_TAKEN))}
        s, need, took = max(c["searches"], 1), max(c["candidate_steps_needed"], 1), c["candidate_steps_taken_by_slowest_lanes"]
        c["candidates_per_search"] = 4.0 * c["candidate_steps_needed"] / s
        c["distance_evaluations"] = 4 * c["candidate_steps_needed"]
        c["lockstep_ratio"] = 64.0 * took / need          # lane slots the trips spent per lane step needed
        c["steps_per_searching_trip"] = took / max(c["wave_trips"] - c["wave_trips_without_a_search"], 1)
        c["steps_per_search"] = c["candidate_steps_needed"] / s
        return c

    def profile_read(self, minmax=False):
        """{kernel name: (launches, total ms)}; minmax=True: (launches, total ms, shortest launch ms, longest launch ms)"""
        buf = (_lib.KernelStatC * 64)()
        n = self._L.tc_profile_read(self._h, buf, 64)
        if minmax:
            return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms), float(buf[i].min_ms), float(buf[i].max_ms)) for i in range(min(n, 64))}
        return {buf[i].name.decode(): (int(buf[i].launches), float(buf[i].total_ms)) for i in range(min(n, 64))}

    # ---- normals ----
    def _cfg(self, config: NormalEstimationConfig):
        c = _lib.NormalConfig()
        self._L.tc_normal_config_default(C.byref(c))
        c.k_neighbors = int(config.k_neighbors)
        if config.radius is not None:
            c.has_radius, c.radius = 1, float(config.radius)
        c.consistent_orientation = 1 if config.consistent_orientation else 0
        if config.viewpoint is not None:
            c.has_viewpoint = 1
            for i in range(3):
                c.viewpoint[i] = float(config.viewpoint[i])
        return c

    def estimate_normals_with_config(self, cloud, config: NormalEstimationConfig):
        """normals.rs:257-357 -> (N, 6) array of NormalPoint3f {position, normal}."""
        c = self._cfg(config)
        x = _points(cloud)
        out = _new(x.device, (x.n, 6))
        fn = self._road(x, self._L.tc_estimate_normals, self._L.tc_estimate_normals_device)
        self._check(fn(self._h, x.ptr, x.n, C.byref(c), _ptr(out)))
        return out

    def estimate_normals_slice(self, cloud, config: NormalEstimationConfig, begin: int, end: int):
        """tc_estimate_normals_slice_device: NormalPoint3f records of the cell-sorted positions [begin, end) of the
        device-resident cloud, in sorted order (one rank's share of a multi-GPU run, threecrate_amd.distributed)."""
        c = self._cfg(config)
        x = _points(cloud, on_device=True)
        out = _new(x.device, (max(end - begin, 0), 6))
        self._order(x.device)
        self._check(self._L.tc_estimate_normals_slice_device(self._h, x.ptr, x.n, C.byref(c), int(begin), int(end), _ptr(out)))
        return out

    def normals_unsort(self, sorted_all):
        """tc_normals_unsort_device: the gathered slices (n, 6, sorted order) -> (n, 6) in input order; uses the index the
        last estimate_normals_slice call left in this context."""
        srt = _points(sorted_all, 6, on_device=True)
        out = _new(srt.device, (srt.n, 6))
        self._order(srt.device)
        self._check(self._L.tc_normals_unsort_device(self._h, srt.ptr, srt.n, _ptr(out)))
        return out

    def estimate_normals(self, cloud, k: int = 10):
        """normals.rs:238-247"""
        return self.estimate_normals_with_config(cloud, NormalEstimationConfig(k_neighbors=k))

    def estimate_normals_radius(self, cloud, radius: float, consistent_orientation: bool):
        """normals.rs:368-380"""
        return self.estimate_normals_with_config(
            cloud, NormalEstimationConfig(k_neighbors=10, radius=radius, consistent_orientation=consistent_orientation))

    def compute_normals(self, points, k: int):
        """GpuContext::compute_normals (threecrate-gpu/src/normals.rs:367-374): normals only (N, 3)."""
        return self.estimate_normals(points, k)[:, 3:]

    # ---- batch k-NN ----
    def find_k_nearest_batch(self, cloud, queries, k: int):
        """gpu_find_k_nearest_batch (threecrate-gpu/src/nearest_neighbor.rs:345-355) /
        KdTree.knn (threecrate-python/src/lib.rs:735-745): (idx (nq,k) int64, dist (nq,k) f32, count (nq,)).
        Rows are ascending by distance; entries past count[q] are undefined."""
        c, q = _as_host(cloud), _as_host(queries)
        idx, dist, cnt = _search_out(None, len(q), k)
        self._check(self._L.tc_knn(self._h, c.ctypes.data, c.shape[0], q.ctypes.data, q.shape[0], int(k), idx.ctypes.data,
                                   dist.ctypes.data, cnt.ctypes.data))
        return idx.astype(np.int64), dist, cnt

    def find_k_nearest(self, cloud, query, k: int):
        """gpu_find_k_nearest (threecrate-gpu/src/nearest_neighbor.rs:332-343): [(index, distance), ...]"""
        return _first_row(*self.find_k_nearest_batch(cloud, _one_query(query), k))

    def find_radius_neighbors_batch(self, cloud, queries, radius: float, k_max: int = 32):
        """find_radius_neighbors (nearest_neighbor.rs:254-298) for many queries, capped at the k_max nearest like
        gpu_find_radius_neighbors (threecrate-gpu/src/nearest_neighbor.rs:357-367): (idx, dist, count)."""
        c, q = _as_host(cloud), _as_host(queries)
        idx, dist, cnt = _search_out(None, len(q), k_max)
        self._check(self._L.tc_radius_search(self._h, c.ctypes.data, c.shape[0], q.ctypes.data, q.shape[0], float(radius), int(k_max),
                                             idx.ctypes.data, dist.ctypes.data, cnt.ctypes.data))
        return idx.astype(np.int64), dist, cnt

    def find_radius_neighbors(self, cloud, query, radius: float, k_max: int = 32):
        """gpu_find_radius_neighbors (threecrate-gpu/src/nearest_neighbor.rs:357-367): [(index, distance), ...]"""
        return _first_row(*self.find_radius_neighbors_batch(cloud, _one_query(query), radius, k_max))

    # ---- voxel grid filter ----
    def voxel_grid_filter(self, cloud, voxel_size: float):
        """filtering.rs:38-133 -> (M, 3) centroids, sorted by voxel key (kx, ky, kz)."""
        n_out = C.c_size_t(0)
        x = _points(cloud)
        out = _new(x.device, (max(1, x.n), 3))
        fn = self._road(x, self._L.tc_voxel_grid_filter, self._L.tc_voxel_grid_filter_device)
        self._check(fn(self._h, x.ptr, x.n, voxel_size, _ptr(out), C.byref(n_out)))
        return out[: n_out.value] if x.is_torch else out[: n_out.value].copy()

    # ---- Euclidean cluster extraction ----
    def extract_euclidean_clusters_labels(self, cloud, tolerance: float, min_cluster_size: int, max_cluster_size: int):
        """segmentation.rs:396-455 -> (labels (n,) uint32, members (n,) uint32, offsets (n_clusters + 1,) uint64).
        labels[i] = rank of point i's cluster (largest first) or TC_CLUSTER_NONE; cluster k is
        members[offsets[k]:offsets[k + 1]], in ascending original index.  Torch device tensors in -> int32 / int64 device
        tensors out (TC_CLUSTER_NONE reads as -1 there)."""
        n_cl = C.c_size_t(0)
        mn, mx = int(min_cluster_size), int(max_cluster_size)
        if mn < 0 or mx < 0:
            raise InvalidData("cluster sizes must not be negative")
        x = _points(cloud)
        n = x.n
        labels, members = _new(x.device, max(1, n), np.uint32), _new(x.device, max(1, n), np.uint32)
        offsets = _new(x.device, n // max(mn, 1) + 1, np.uint64, zeros=not x.is_torch)
        fn = self._road(x, self._L.tc_extract_euclidean_clusters, self._L.tc_extract_euclidean_clusters_device)
        self._check(fn(self._h, x.ptr, n, float(tolerance), mn, mx, _ptr(labels), _ptr(members), _ptr(offsets), C.byref(n_cl)))
        offsets = offsets[: n_cl.value + 1]
        if x.is_torch:
            return labels[:n], members[: int(offsets[-1])], offsets
        offsets = offsets.copy()
        return labels[:n], members[: int(offsets[-1])].copy(), offsets

    def extract_euclidean_clusters(self, cloud, tolerance: float, min_cluster_size: int, max_cluster_size: int):
        """extract_euclidean_clusters (segmentation.rs:396-455): a list of index arrays (int64), largest cluster first,
        equal sizes by smallest index; indices inside a cluster ascending.  Torch device tensors in -> torch tensors out."""
        _, members, offsets = self.extract_euclidean_clusters_labels(cloud, tolerance, min_cluster_size, max_cluster_size)
        if _is_torch(members):
            o = offsets.cpu().tolist()
            m = members.long()
            return [m[o[k]:o[k + 1]] for k in range(len(o) - 1)]
        o = offsets.astype(np.int64)
        m = members.astype(np.int64)
        return [m[o[k]:o[k + 1]] for k in range(len(o) - 1)]

    # ---- outlier removal (include/threecrate_hip_filters.h) ----
    def _outliers(self, cloud, host_fn, dev_fn, params, want_index, want_mean=None, want_threshold=False):
        """One call of an outlier filter -> OutlierResult, the kept arrays sliced to the count (numpy in -> numpy out, torch device
        tensor in -> torch out; kept indices are uint32, int32 on the device).  An output nobody asked for is not allocated: the
        library takes NULL for it.  want_mean None: the entry point has no mean_distance argument (the radius filter)."""
        x = _points(cloud)
        cap = max(1, x.n)
        out = _new(x.device, (cap, 3))
        index = _new(x.device, cap, np.uint32) if want_index else None
        mean = _new(x.device, cap) if want_mean else None
        n_out, thr = C.c_size_t(0), C.c_float(0.0)
        tail = ([_ptr(mean) if want_mean else None] if want_mean is not None else []) + [C.byref(n_out)] + ([C.byref(thr)] if want_threshold else [])
        self._check(self._road(x, host_fn, dev_fn)(self._h, x.ptr, x.n, *params, _ptr(out), _ptr(index) if want_index else None, *tail))
        m = n_out.value
        cut = (lambda a: a[:m]) if x.is_torch else (lambda a: a[:m].copy())
        return OutlierResult(cut(out), cut(index) if want_index else None, mean[: x.n] if want_mean else None,
                             thr.value if want_threshold and x.n else None)

    @staticmethod
    def _neighbour_count(k, what):
        k = int(k)
        if k < 0:
            raise InvalidData(f"{what} must not be negative")
        return k

    @staticmethod
    def _pick(r, return_index, return_mean_distance=False):
        got = (r.points,) + ((r.index,) if return_index else ()) + ((r.mean_distance,) if return_mean_distance else ())
        return got[0] if len(got) == 1 else got

    def _sor(self, cloud, k_neighbors, std_dev_multiplier, want_index, want_mean):
        L = self._L
        return self._outliers(cloud, L.tc_statistical_outlier_removal, L.tc_statistical_outlier_removal_device,
                              (self._neighbour_count(k_neighbors, "k_neighbors"), float(std_dev_multiplier)), want_index, bool(want_mean), True)

    def statistical_outlier_removal_detailed(self, cloud, k_neighbors: int, std_dev_multiplier: float):
        """statistical_outlier_removal (filtering.rs:249-321) with everything the entry point returns ->
        OutlierResult(points, index, mean_distance, threshold): the kept points in input order, their original indices, every
        input point's mean distance to its k nearest (NaN for a point with a non-finite coordinate), and threshold_used, the
        value the means were compared with (None for an empty cloud).  The only road to the threshold from Python."""
        return self._sor(cloud, k_neighbors, std_dev_multiplier, True, True)

    def statistical_outlier_removal(self, cloud, k_neighbors: int, std_dev_multiplier: float, return_index=False, return_mean_distance=False):
        """statistical_outlier_removal (filtering.rs:249-321): the (M, 3) kept points in input order [, their indices] [, the (n,) mean
        distances]."""
        return self._pick(self._sor(cloud, k_neighbors, std_dev_multiplier, return_index, return_mean_distance), return_index, return_mean_distance)

    def statistical_outlier_removal_with_threshold(self, cloud, k_neighbors: int, threshold: float, return_index=False, return_mean_distance=False):
        """statistical_outlier_removal_with_threshold (filtering.rs:335-395): keeps the points whose mean distance is <= threshold."""
        L = self._L
        r = self._outliers(cloud, L.tc_statistical_outlier_removal_with_threshold, L.tc_statistical_outlier_removal_with_threshold_device,
                           (self._neighbour_count(k_neighbors, "k_neighbors"), float(threshold)), return_index, bool(return_mean_distance))
        return self._pick(r, return_index, return_mean_distance)

    def radius_outlier_removal(self, cloud, radius: float, min_neighbors: int, return_index=False):
        """radius_outlier_removal (filtering.rs:167-213): keeps the points with at least min_neighbors other points within radius."""
        L = self._L
        r = self._outliers(cloud, L.tc_radius_outlier_removal, L.tc_radius_outlier_removal_device,
                           (float(radius), self._neighbour_count(min_neighbors, "min_neighbors")), return_index)
        return self._pick(r, return_index)

    # ---- RANSAC plane segmentation (include/threecrate_hip_segmentation.h) ----
    def _plane(self, x, host_fn, dev_fn, threshold, params, iterations, return_index):
        index = _new(x.device, max(1, x.n), np.uint32) if return_index else None
        coeff = (C.c_float * 4)()
        n_in, best = C.c_size_t(0), C.c_uint32(0)
        self._check(self._road(x, host_fn, dev_fn)(self._h, x.ptr, x.n, float(threshold), *params, coeff, _ptr(index) if return_index else None,
                                                   C.byref(n_in), C.byref(best)))
        m = n_in.value
        if return_index:
            index = index[:m] if x.is_torch else index[:m].copy()
        return PlaneSegmentationResult(np.array(coeff[:], np.float32), index, iterations, best.value, m)

    def segment_plane(self, cloud, threshold: float, max_iters: int, seed: int = 0, return_index=True):
        """segment_plane (segmentation.rs:117-180) -> PlaneSegmentationResult.  The triples come from the facade's deterministic
        generator (threecrate-gpu/src/segmentation.rs:979-1011) with `seed` XORed into its initial state (0: the facade's own
        sequence), so a call is reproducible; among equal scores the lowest iteration wins.  return_index=False skips the
        inlier list (inlier_indices is None, num_inliers is still the winner's score)."""
        iters = int(max_iters)
        if iters < 0:
            raise InvalidData("max_iters must not be negative")
        L = self._L
        return self._plane(_points(cloud), L.tc_segment_plane, L.tc_segment_plane_device, threshold,
                           (iters, int(seed) & 0xFFFFFFFFFFFFFFFF), iters, return_index)

    def segment_plane_samples(self, cloud, threshold: float, samples, return_index=True):
        """The same scoring over the caller's own triples: `samples` is (n_samples, 3) point indices (uint32; an int32 device tensor
        with a device cloud).  A row with an index >= n, a repeated point or three collinear points is a candidate without a
        model.  best_iteration is the winning row."""
        x = _points(cloud)
        if x.is_torch:
            import torch
            smp = samples.detach().to(device=x.device, dtype=torch.int32).contiguous().reshape(-1, 3)      # a host tensor moves to the cloud's device
        else:
            smp = np.ascontiguousarray(np.asarray(samples, dtype=np.uint32)).reshape(-1, 3)
        L = self._L
        return self._plane(x, L.tc_segment_plane_samples, L.tc_segment_plane_samples_device, threshold, (_ptr(smp), smp.shape[0]),
                           smp.shape[0], return_index)

    # ---- global registration: matching and RANSAC (include/threecrate_hip_global.h, the companion library), and the pipeline ----
    def _global(self):
        if getattr(self, "_G", None) is None:
            self._G = _lib.load_companion("threecrate_hip_global.h")
        return self._G

    def match_features(self, src_desc, tgt_desc, return_distance=False):
        """find_feature_correspondences (global_registration.rs:85-110): for every row of src_desc (ns, 33) the index of the nearest row
        of tgt_desc (nt, 33) by squared L2 distance, the lowest index among equals -> (ns,) uint32 [int32 on the device]; with
        return_distance also the winning squared distances.  The correspondences are (i, index[i])."""
        dim = int(src_desc.shape[1]) if getattr(src_desc, "ndim", 0) == 2 else _lib.TC_FPFH_DIM
        if getattr(tgt_desc, "ndim", 0) == 2 and int(tgt_desc.shape[1]) != dim:
            raise InvalidData("source and target descriptors differ in length")
        G = self._global()
        s = _points(src_desc, max(dim, 1))
        t = _points(tgt_desc, max(dim, 1), on_device=s.is_torch)
        index = _new(s.device, max(1, s.n), np.uint32)
        dist = _new(s.device, max(1, s.n)) if return_distance else None
        fn = self._road(s, G.tc_match_features, G.tc_match_features_device)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, dim, _ptr(index), _ptr(dist) if return_distance else None))
        if s.is_torch:
            self._release(s.device)                 # the device entry point returns with its kernel enqueued: torch's stream waits for it
        return (index[:s.n], dist[:s.n]) if return_distance else index[:s.n]

    def ransac_correspondences(self, source, target, corr_src, corr_tgt, threshold, inlier_ratio=0.25, max_iterations=50_000, seed=0,
                               samples=None, candidates=False) -> "RansacResult":
        """The RANSAC loop of global_registration_with_normals (global_registration.rs:252-299) over the pairs
        (source[corr_src[p]], target[corr_tgt[p]]) -> RansacResult.  The triples come from a seeded generator on the device, or from
        `samples` ((n, 3) correspondence indices).  candidates=True also returns every candidate's transform and score."""
        G = self._global()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        cs, ct = _u32(corr_src, s), _u32(corr_tgt, s)
        if cs.shape[0] != ct.shape[0]:
            raise InvalidData("corr_src and corr_tgt differ in length")
        m = int(cs.shape[0])
        if samples is None:
            n_cand = int(max_iterations)
            if n_cand < 0:
                raise InvalidData("max_iterations must not be negative")
            params = (n_cand, int(seed) & 0xFFFFFFFFFFFFFFFF)
            host_fn, dev_fn = G.tc_ransac_correspondences, G.tc_ransac_correspondences_device
        else:
            smp = _u32(samples, s, 3)
            n_cand = int(smp.shape[0])
            params = (_ptr(smp), n_cand)
            host_fn, dev_fn = G.tc_ransac_correspondences_samples, G.tc_ransac_correspondences_samples_device
        want = candidates and n_cand <= _lib.TC_RANSAC_MAX_ITERS
        cand_t = _new(s.device, (max(1, n_cand), 12)) if want else None
        cand_c = _new(s.device, max(1, n_cand), np.uint32) if want else None
        T, r = (C.c_float * 12)(), _lib.RansacResultC()
        fn = self._road(s, host_fn, dev_fn)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, _ptr(cs), _ptr(ct), m, float(threshold), float(inlier_ratio), *params, T, C.byref(r),
                       _ptr(cand_t) if want else None, _ptr(cand_c) if want else None))
        return RansacResult(np.array(T[:], np.float32), int(r.inlier_count), float(r.inlier_ratio), int(r.iterations_run), int(r.best_iteration),
                            bool(r.early_exit), cand_t[:n_cand] if want else None, cand_c[:n_cand] if want else None)

    def global_registration(self, source, target, config: "GlobalRegistrationConfig" = None, source_normals=None, target_normals=None):
        """global_registration / global_registration_with_normals (global_registration.rs:185-333) -> GlobalRegistrationResult, composed
        of public calls: (1) estimate_normals unless the (n, 6) NormalPoint3f records (or (n, 3) normals) are given, (2)
        extract_fpfh_features_with_normals of both clouds, (3) match_features, (4) ransac_correspondences over the records' positions,
        (5) with refine_with_icp, icp_point_to_point from RANSAC's pose (its rotation as a quaternion, converted on the host in f64).
        One deviation: ransac_iterations = 0 is InvalidData ("Max iterations must be positive", the C contract's check); the reference
        runs no iteration, keeps the identity and goes on to ICP."""
        cfg = config or GlobalRegistrationConfig()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        if s.n == 0:
            raise AlgorithmError("Source point cloud is empty")
        if t.n == 0:
            raise AlgorithmError("Target point cloud is empty")

        def records(x, normals):
            if normals is None:
                return self.estimate_normals(x.a, cfg.normal_k_neighbors)
            n = _points(normals, 6 if normals.shape[-1] == 6 else 3, on_device=x.is_torch)
            if n.a.shape[1] == 6:
                return n.a
            if n.n != x.n:
                raise InvalidData("normals length must equal the number of points")
            if x.is_torch:
                import torch
                return torch.cat([x.a, n.a], dim=1)
            return np.concatenate([x.a, n.a], axis=1)
        sn, tn = records(s, source_normals), records(t, target_normals)
        sd = self.extract_fpfh_features_with_normals(sn, cfg.fpfh_radius, cfg.fpfh_k_neighbors)
        td = self.extract_fpfh_features_with_normals(tn, cfg.fpfh_radius, cfg.fpfh_k_neighbors)
        match = self.match_features(sd, td)
        m = int(match.shape[0])
        if m < 3:
            raise AlgorithmError("Too few feature correspondences for RANSAC (need ≥ 3)")
        if s.is_torch:
            import torch
            arange = torch.arange(m, dtype=torch.int32, device=s.device)
        else:
            arange = np.arange(m, dtype=np.uint32)
        rr = self.ransac_correspondences(sn[:, 0:3], tn[:, 0:3], arange, match, cfg.distance_threshold, cfg.inlier_ratio, cfg.ransac_iterations,
                                         cfg.seed)
        init = rotation_to_isometry(rr.transform)
        icp = None
        if cfg.refine_with_icp:
            icp = self.icp_point_to_point(s.a, t.a, init, cfg.icp_max_iterations, 1e-6, cfg.icp_distance_threshold, correspondences=False)
        return GlobalRegistrationResult(icp.transformation if icp is not None else init, rr.inlier_count, rr.inlier_ratio, icp, rr)

    # ---- NDT registration (include/threecrate_hip_ndt.h) ----
    def ndt_registration(self, source, target, init=None, resolution=1.0, step_size=0.1, max_iterations=35, epsilon=1e-4,
                         min_points_per_voxel=5) -> "NdtResult":
        """ndt_registration (ndt_registration.rs:188-260) -> NdtResult.  numpy arrays take the host entry point, torch device tensors
        the device one; the first array chooses the road."""
        iters, min_pts = int(max_iterations), int(min_points_per_voxel)
        if iters < 0 or min_pts < 0:
            raise InvalidData("max_iterations and min_points_per_voxel must not be negative")
        c = _lib.NdtConfigC(float(resolution), float(step_size), iters, float(epsilon), min_pts)
        i7, r = _init7(init), _lib.NdtResultC()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        fn = self._road(s, self._L.tc_ndt_registration, self._L.tc_ndt_registration_device)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, C.byref(c), C.byref(r)))
        return NdtResult(np.array(r.transformation[:], np.float32), float(r.score), int(r.iterations), bool(r.converged), int(r.n_voxels),
                         int(r.n_hits))

    def ndt_voxels(self, target, resolution: float, min_points_per_voxel: int = 5):
        """The voxel map ndt_registration builds from `target` -> (keys (V, 3) int32, counts (V,) uint32 [int32 on the device], mean
        (V, 3), inv_cov (V, 6): xx xy xz yy yz zz), voxels in ascending (kx, ky, kz) order."""
        min_pts = int(min_points_per_voxel)
        if min_pts < 0:
            raise InvalidData("min_points_per_voxel must not be negative")
        t = _points(target)
        fn = self._road(t, self._L.tc_ndt_voxels, self._L.tc_ndt_voxels_device)
        cap, nv = t.n // max(min_pts, 1), C.c_size_t(0)         # a voxel holds at least max(min_points, 1) points
        keys, counts, mean, inv_cov = _new(t.device, (cap, 3), np.uint32), _new(t.device, cap, np.uint32), _new(t.device, (cap, 3)), _new(t.device, (cap, 6))
        self._check(fn(self._h, t.ptr, t.n, float(resolution), min_pts, _ptr(keys), _ptr(counts), _ptr(mean), _ptr(inv_cov), cap, C.byref(nv)))
        cut = (lambda a: a[:nv.value]) if t.is_torch else (lambda a: a[:nv.value].copy())
        keys, counts, mean, inv_cov = cut(keys), cut(counts), cut(mean), cut(inv_cov)
        if not t.is_torch:
            keys = keys.view(np.int32)
        return keys, counts, mean, inv_cov

    # ---- TSDF volumes (include/threecrate_hip_tsdf.h) ----
    def tsdf_volume(self, voxel_size, truncation_distance, resolution, origin=(0, 0, 0), max_weight=100) -> "TsdfVolume":
        """a dense TSDF volume in device memory (TsdfVolumeGpu::new, tsdf.rs:551-586), in its initial state"""
        return TsdfVolume(self, voxel_size, truncation_distance, resolution, origin, max_weight)

    # ---- streaming voxel map (include/threecrate_hip_voxelmap.h, the second companion library) ----
    def voxel_map(self, voxel_size, initial_capacity=0) -> "VoxelMap":
        """an empty voxel map in device memory (StreamingVoxelFilter::new, streaming.rs:224-229)"""
        return VoxelMap(self, voxel_size, initial_capacity)

    # ---- mesh smoothing ----
    _MESH_METHODS = {"laplacian": _lib.TC_MESH_LAPLACIAN, "taubin": _lib.TC_MESH_TAUBIN, "hc": _lib.TC_MESH_HC}

    def smooth_mesh(self, vertices, faces, method="laplacian", iterations=10, lambda_=0.5, mu=-0.53, alpha=0.0, beta=0.5):
        """Smooth a triangle mesh (tc_mesh_smooth, the companion library of include/threecrate_hip_mesh.h): `iterations` sweeps of
        "laplacian" (lambda_), "taubin" (lambda_, then mu) or "hc" (alpha, beta) over the one-ring adjacency of `faces` (m x 3 vertex
        indices), neighbours summed in ascending index order.  numpy vertices take the host entry point, a torch device tensor the
        device one; the faces follow the vertices.  -> the smoothed vertices (n, 3) float32, of the input's kind."""
        L = _lib.load_companion("threecrate_hip_mesh.h")
        code = self._MESH_METHODS.get(method, method)
        if not isinstance(code, int) or isinstance(code, bool) or not 0 <= code < 2 ** 32 or not 0 <= int(iterations) < 2 ** 32:
            raise InvalidData('method is "laplacian", "taubin" or "hc"; iterations fits 32 bits')
        p = _points(vertices)
        f = _u32(faces, p, 3)
        if p.n == 0 or f.shape[0] == 0:             # the library's check (2), made here: an empty array has no address to pass
            raise InvalidData("Mesh is empty")
        cfg = _lib.MeshSmoothConfigC(code, int(iterations), float(lambda_), float(mu), float(alpha), float(beta))
        out = _new(p.device, (p.n, 3))
        fn = self._road(p, L.tc_mesh_smooth, L.tc_mesh_smooth_device)
        self._check(fn(self._h, p.ptr, p.n, _ptr(f), f.shape[0], C.byref(cfg), _ptr(out)))
        return out

    def mesh_adjacency(self, n_vertices, faces):
        """The one-ring vertex adjacency of `faces` as a CSR (tc_mesh_vertex_adjacency): count, then fill.
        -> offsets (n_vertices + 1,), neighbors (offsets[-1],), uint32 (int32 bits for a torch device tensor); the neighbours of
        vertex i are neighbors[offsets[i]:offsets[i + 1]], ascending."""
        L = _lib.load_companion("threecrate_hip_mesh.h")
        like = _road_of(faces)
        f = _u32(faces, like, 3)
        if int(n_vertices) <= 0 or f.shape[0] == 0:
            raise InvalidData("Mesh is empty")
        fn = self._road(like, L.tc_mesh_vertex_adjacency, L.tc_mesh_vertex_adjacency_device)
        n, total = int(n_vertices), C.c_size_t(0)
        self._check(fn(self._h, n, _ptr(f), f.shape[0], None, None, 0, C.byref(total)))
        offsets, neighbors = _new(like.device, n + 1, np.uint32), _new(like.device, max(total.value, 1), np.uint32)
        self._check(fn(self._h, n, _ptr(f), f.shape[0], _ptr(offsets), _ptr(neighbors), total.value, C.byref(total)))
        return offsets, neighbors[:total.value]

    # ---- mesh simplification ----
    _SIMPLIFY_STRATEGIES = {"centroid": _lib.TC_SIMPLIFY_CENTROID, "weighted_average": _lib.TC_SIMPLIFY_WEIGHTED_AVERAGE}
    SIMPLIFY_DEFAULT_FEATURE_ANGLE = float(np.float32(45.0) * (np.float32(np.pi) / np.float32(180.0)))     # 45.0f32.to_radians()

    def simplify_mesh_clustering(self, vertices, faces, reduction_ratio, strategy="centroid", preserve_boundary=True,
                                 feature_angle_threshold=SIMPLIFY_DEFAULT_FEATURE_ANGLE, normals=None, colors=None, return_map=False):
        """Simplify a triangle mesh by vertex clustering (tc_simplify_clustering, the companion library of
        include/threecrate_hip_simplify.h; ClusteringSimplifier's uniform road): one representative per grid cell and class (boundary,
        feature, interior), "centroid" or "weighted_average" (by valence); degenerate and repeated faces dropped.  normals (n, 3) float32
        and colors (n, 3) uint8 are carried through.  numpy vertices take the host entry point, a torch device tensor the device one;
        the other arrays follow the vertices.  The outputs are allocated at the input's sizes, which bound the counts: one call.
        -> (vertices, faces[, normals][, colors][, map]) of the input's kind; map[i] is the output vertex of input vertex i, 0xFFFFFFFF
        when its cluster is in no surviving face.  "minimum_error" (nalgebra's inverse) and adaptive clustering (a sequential octree)
        are not served: Unsupported."""
        L = _lib.load_companion("threecrate_hip_simplify.h")
        if strategy == "minimum_error":
            raise Unsupported("simplify_mesh_clustering: the minimum-error representative is not supported by the HIP backend")
        code = self._SIMPLIFY_STRATEGIES.get(strategy, strategy)
        if not isinstance(code, int) or isinstance(code, bool) or not 0 <= code < 2 ** 32:
            raise InvalidData('strategy is "centroid" or "weighted_average"')
        p = _points(vertices)
        f = _u32(faces, p, 3)
        if p.n == 0 or f.shape[0] == 0:             # the library's check (2), made here: an empty array has no address to pass
            raise InvalidData("Mesh is empty")
        n, m = p.n, f.shape[0]
        nrm = col = out_n = out_c = out_map = None
        if normals is not None:
            nrm = _points(normals, on_device=p.is_torch)
            if nrm.n != n:
                raise InvalidData("simplify_mesh_clustering: normals must have one row per vertex")
            out_n = _new(p.device, (n, 3))
        if colors is not None:
            if p.is_torch:
                import torch
                col = colors.detach().to(device=p.device, dtype=torch.uint8).contiguous().reshape(-1, 3)
            else:
                col = np.ascontiguousarray(np.asarray(colors, dtype=np.uint8)).reshape(-1, 3)
            if col.shape[0] != n:
                raise InvalidData("simplify_mesh_clustering: colors must have one row per vertex")
            out_c = _new(p.device, (n, 3), np.uint8)
        if return_map:
            out_map = _new(p.device, n, np.uint32)
        cfg = _lib.SimplifyConfigC(code, int(bool(preserve_boundary)), float(feature_angle_threshold), float(reduction_ratio))
        out_v, out_f = _new(p.device, (n, 3)), _new(p.device, (m, 3), np.uint32)
        nv, nf = C.c_size_t(0), C.c_size_t(0)
        opt = lambda a: None if a is None else _ptr(a)
        fn = self._road(p, L.tc_simplify_clustering, L.tc_simplify_clustering_device)
        self._check(fn(self._h, p.ptr, n, _ptr(f), m, None if nrm is None else nrm.ptr, opt(col), C.byref(cfg), _ptr(out_v), opt(out_n), opt(out_c), n,
                       _ptr(out_f), m, opt(out_map), C.byref(nv), C.byref(nf)))
        out = [out_v[:nv.value], out_f[:nf.value]]
        if out_n is not None:
            out.append(out_n[:nv.value])
        if out_c is not None:
            out.append(out_c[:nv.value])
        if out_map is not None:
            out.append(out_map)
        return tuple(out)

    def simplify_mesh_quadric(self, vertices, faces, reduction_ratio=0.5, preserve_boundary=True, max_edge_length=None, return_map=False,
                              device=None):
        """Simplify a triangle mesh by quadric-error edge collapse (tc_simplify_quadric, the companion library of
        include/threecrate_hip_qem.h; QuadricErrorSimplifier, what the wheel's simplify_mesh runs): rounds of independent collapses,
        cheapest first, until (1 - reduction_ratio) of the faces are left or no edge may collapse.  max_edge_length: None is no limit
        (0 means the same to the library), else longer edges do not collapse.  numpy vertices take the host entry point, a torch device
        tensor the device one; the faces follow the vertices.  device: a torch device to move numpy input to first (the device road,
        torch outputs); None: the input's own kind.  The outputs are allocated at the input's sizes, which bound the counts: one call.
        -> (vertices, faces[, map]) of the input's kind; map[i] is the output vertex that input vertex i ended in, 0xFFFFFFFF when that
        vertex is in no surviving face.  No normals or colours, as in the reference.  The number of rounds that collapsed something is
        left in self.last_qem_rounds."""
        L = _lib.load_companion("threecrate_hip_qem.h")
        if device is not None and not _is_torch(vertices):
            import torch
            vertices = torch.from_numpy(_as_host(vertices)).to(device)
        p = _points(vertices)
        f = _u32(faces, p, 3)
        if p.n == 0 or f.shape[0] == 0:             # the library's check (2), made here: an empty array has no address to pass
            raise InvalidData("Mesh is empty")
        n, m = p.n, f.shape[0]
        cfg = _lib.QemConfigC(float(reduction_ratio), int(bool(preserve_boundary)), 0.0 if max_edge_length is None else float(max_edge_length))
        out_v, out_f = _new(p.device, (n, 3)), _new(p.device, (m, 3), np.uint32)
        out_map = _new(p.device, n, np.uint32) if return_map else None
        nv, nf, rounds = C.c_size_t(0), C.c_size_t(0), C.c_uint32(0)
        fn = self._road(p, L.tc_simplify_quadric, L.tc_simplify_quadric_device)
        self._check(fn(self._h, p.ptr, n, _ptr(f), m, C.byref(cfg), _ptr(out_v), n, _ptr(out_f), m, None if out_map is None else _ptr(out_map),
                       C.byref(nv), C.byref(nf), C.byref(rounds)))
        self.last_qem_rounds = int(rounds.value)
        out = (out_v[:nv.value], out_f[:nf.value])
        return out + (out_map,) if return_map else out

    # ---- alpha-shape reconstruction ----
    _ALPHA_MODES = {"boundary": _lib.TC_ALPHA_BOUNDARY_ONLY, "full": _lib.TC_ALPHA_FULL}

    def alpha_shape(self, points, alpha, mode="boundary", min_triangle_area=1e-8, max_triangles=50000, return_stats=False, fast_mode=False):
        """The alpha shape of a cloud as triangles over its own points (tc_alpha_shape, the companion library of
        include/threecrate_hip_alpha.h; alpha_shape_reconstruction's quality road): every index-ordered triple inside a ball of radius
        alpha around its lowest point that passes the reference's geometric test is a candidate; "boundary" keeps the candidates with
        an edge no other candidate shares, "full" all of them, both with a circumradius of at most alpha.  max_triangles: the reference
        stops after 50 000 candidates in index order (the default, for the reference's mesh); 0 lifts the cap.  fast_mode and the
        "adaptive" mode are not served: Unsupported.  numpy points take the host entry point, a torch device tensor the device one.  Two
        calls: the counts, then the faces.
        -> faces (m, 3) uint32 (int32 bits for a torch device tensor) indexing `points` [, stats: a dict of candidates,
        boundary_candidates, faces, capped]."""
        L = _lib.load_companion("threecrate_hip_alpha.h")
        if fast_mode:
            raise Unsupported("alpha_shape: fast_mode is not supported by the HIP backend")
        if mode == "adaptive":
            raise Unsupported("alpha_shape: the adaptive mode is not supported by the HIP backend (boundary or full)")
        code = self._ALPHA_MODES.get(mode, mode)
        if not isinstance(code, int) or isinstance(code, bool) or not 0 <= code < 2 ** 32 or not 0 <= int(max_triangles) < 2 ** 32:
            raise InvalidData('mode is "boundary" or "full"; max_triangles fits 32 bits')
        p = _points(points)
        if p.n == 0:                                # the library's check (2), made here: an empty array has no address to pass
            raise InvalidData("Point cloud is empty")
        cfg = _lib.AlphaConfigC(float(alpha), code, float(min_triangle_area), int(max_triangles))
        st = _lib.AlphaStatsC()
        fn = self._road(p, L.tc_alpha_shape, L.tc_alpha_shape_device)
        self._check(fn(self._h, p.ptr, p.n, C.byref(cfg), None, 0, C.byref(st)))
        faces = _new(p.device, (int(st.faces), 3), np.uint32)
        if p.is_torch:
            self._order(p.device)                   # the output was made on torch's stream
        self._check(fn(self._h, p.ptr, p.n, C.byref(cfg), _ptr(faces), int(st.faces), C.byref(st)))
        if not return_stats:
            return faces
        return faces, {"candidates": int(st.candidates), "boundary_candidates": int(st.boundary_candidates), "faces": int(st.faces), "capped": int(st.capped)}

    # ---- ground segmentation ----
    GROUND_PATCH_DTYPE = np.dtype([("count", np.uint32), ("n_inliers", np.uint32), ("status", np.uint32), ("normal", np.float32, (3,)),
                                   ("d", np.float32), ("mean_z", np.float32), ("flatness", np.float32)])

    @staticmethod
    def ground_config(sensor_height=1.723, **fields):
        """tc_ground_config: PatchworkConfig::default() with the given sensor height, then the named fields replaced.  zone_radii, num_rings
        (or num_rings_per_zone) and num_sectors (or num_sectors_per_zone) are lists; their lengths give n_zones (lengths that do not fit
        each other are InvalidData with the reference's messages, more than TC_GROUND_MAX_ZONES zones are the library's to refuse)."""
        cfg = _lib.GroundConfigC()
        _lib.load_companion("threecrate_hip_ground.h").tc_ground_config_default(float(sensor_height), C.byref(cfg))
        alias = {"num_rings_per_zone": "num_rings", "num_sectors_per_zone": "num_sectors"}
        fields = {alias.get(k, k): v for k, v in fields.items()}
        lists = {k: list(fields.pop(k)) for k in ("zone_radii", "num_rings", "num_sectors") if k in fields}
        if lists:
            if set(lists) != {"zone_radii", "num_rings", "num_sectors"}:
                raise InvalidData("zone_radii, num_rings and num_sectors are given together")
            nz = len(lists["num_rings"])
            if nz == 0:
                raise InvalidData("num_rings_per_zone must be non-empty")
            if len(lists["zone_radii"]) != nz + 1:
                raise InvalidData("zone_radii.len() must equal num_rings_per_zone.len() + 1")
            if len(lists["num_sectors"]) != nz:
                raise InvalidData("num_sectors_per_zone.len() must equal num_rings_per_zone.len()")
            cfg.n_zones = min(nz, 2 ** 32 - 1)
            kept = min(nz, _lib.TC_GROUND_MAX_ZONES)
            cfg.zone_radii[:] = [float(v) for v in lists["zone_radii"][:kept + 1]] + [0.0] * (_lib.TC_GROUND_MAX_ZONES - kept)
            for name in ("num_rings", "num_sectors"):
                getattr(cfg, name)[:] = [min(int(v), 2 ** 32 - 1) for v in lists[name][:kept]] + [0] * (_lib.TC_GROUND_MAX_ZONES - kept)
        known = {name for name, _ in _lib.GroundConfigC._fields_}
        for k, v in fields.items():
            if k not in known or k == "n_zones":
                raise InvalidData(f"ground_config: unknown field {k}")
            setattr(cfg, k, float(v) if dict(_lib.GroundConfigC._fields_)[k] is C.c_float else min(int(v), 2 ** 32 - 1))
        return cfg

    def segment_ground(self, points, sensor_height=None, config=None, return_points=False, return_index=True, return_patches=True):
        """Split an outdoor LiDAR frame into ground and non-ground points (tc_segment_ground, the companion library of
        include/threecrate_hip_ground.h; patchwork_plus_plus / segment_ground of the reference): concentric zones, rings and sectors cut
        the plane around the sensor into patches, each patch is fitted with a plane (seeds, PCA, inliers, a few times over) and the plane
        is tested for uprightness, elevation and flatness.  config: a tc_ground_config from ground_config(); None: the defaults with
        sensor_height (1.723 when that is None too).  numpy points take the host entry point, a torch device tensor the device one.
        -> a dict: labels (n, bool), n_ground, and as asked for ground / nonground (index arrays, ascending; uint32, int32 bits for a
        torch tensor), ground_points / nonground_points, patches (a structured array of GROUND_PATCH_DTYPE, one record per patch of the
        configuration in (zone, ring, sector) order)."""
        L = _lib.load_companion("threecrate_hip_ground.h")
        if config is None:
            config = self.ground_config(1.723 if sensor_height is None else sensor_height)
        elif sensor_height is not None:
            raise InvalidData("segment_ground: sensor_height and config are given together")
        p = _points(points)
        n = p.n
        n_patches = int(L.tc_ground_patch_count(C.byref(config)))
        want_index = return_index or return_points
        labels = _new(p.device, max(n, 1), np.uint8)
        ground = _new(p.device, max(n, 1), np.uint32) if want_index else None
        nonground = _new(p.device, max(n, 1), np.uint32) if want_index else None
        patches = _new(p.device, (max(n_patches, 1), self.GROUND_PATCH_DTYPE.itemsize), np.uint8) if return_patches else None
        ng = C.c_size_t(0)
        fn = self._road(p, L.tc_segment_ground, L.tc_segment_ground_device)
        self._check(fn(self._h, p.ptr if n else None, n, C.byref(config), _ptr(labels), None if ground is None else _ptr(ground),
                       None if nonground is None else _ptr(nonground), None if patches is None else _ptr(patches), C.byref(ng)))
        k = int(ng.value)
        out = {"labels": labels[:n] != 0, "n_ground": k}
        if want_index:
            out["ground"], out["nonground"] = ground[:k], nonground[:n - k]
        if return_points:
            index = (lambda a: a.long()) if p.is_torch else (lambda a: a.astype(np.int64))
            out["ground_points"], out["nonground_points"] = p.a[index(out["ground"])], p.a[index(out["nonground"])]
        if return_patches:
            raw = patches.cpu().numpy() if p.is_torch else patches
            out["patches"] = np.ascontiguousarray(raw[:n_patches]).view(self.GROUND_PATCH_DTYPE).reshape(-1)
        return out

    # ---- marching cubes ----
    _MC_LAYOUTS ={"z_fastest": _lib.TC_MC_Z_FASTEST, "x_fastest": _lib.TC_MC_X_FASTEST}

    def marching_cubes(self, values, dims=None, voxel_size=(1.0, 1.0, 1.0), origin=(0.0, 0.0, 0.0), iso_level=0.0, normals=True, weld=False,
                       valid=None, layout="z_fastest"):
        """The iso surface of a scalar grid as a triangle mesh (tc_marching_cubes, the companion library of include/threecrate_hip_mc.h;
        MarchingCubes::extract_isosurface).  values: dims[0] * dims[1] * dims[2] floats in `layout`: "z_fastest" (values[x][y][z], the
        reference's; a 3-D array gives dims itself) or "x_fastest" (a TSDF volume's order; a 3-D array is shaped (nz, ny, nx)).
        voxel_size: a number or three.  valid: one byte per voxel, zero = not usable.  weld=False is the reference's layout (a vertex per
        crossing edge per cube); weld=True gives one vertex per grid edge, what smooth_mesh and simplify_mesh_clustering need.
        numpy values take the host entry point, a torch device tensor the device one; valid follows.  Two calls: the counts, then the mesh.
        -> (vertices (n, 3) f32, normals (n, 3) f32 or None, faces (m, 3) uint32 (int32 bits for a torch device tensor))."""
        L = _lib.load_companion("threecrate_hip_mc.h")
        code = self._MC_LAYOUTS.get(layout, layout)
        if not isinstance(code, int) or isinstance(code, bool) or not 0 <= code < 2 ** 32:
            raise InvalidData('layout is "z_fastest" or "x_fastest"')
        if dims is None:
            if len(values.shape) != 3:
                raise InvalidData("marching_cubes: give dims, or values as a 3-D array")
            dims = tuple(values.shape) if code == _lib.TC_MC_Z_FASTEST else tuple(values.shape)[::-1]
        dims = [int(d) for d in dims]
        if len(dims) != 3 or min(dims) < 0 or max(dims) >= 2 ** 32:
            raise InvalidData("marching_cubes: dims has three entries, each fits 32 bits")
        vs = [float(voxel_size)] * 3 if np.ndim(voxel_size) == 0 else [float(v) for v in voxel_size]
        org = [float(o) for o in origin]
        if len(vs) != 3 or len(org) != 3:
            raise InvalidData("marching_cubes: voxel_size and origin have three entries")
        nvox = dims[0] * dims[1] * dims[2]
        v = _image(values, np.float32, nvox, "values")
        if valid is not None and v.is_torch and not _is_torch(valid):
            import torch
            valid = torch.from_numpy(np.ascontiguousarray(np.asarray(valid) != 0).view(np.uint8)).to(v.device)
        m = None if valid is None else _image(valid, np.uint8, nvox, "valid", on_device=v.is_torch)
        grid = _lib.McGridC((C.c_uint32 * 3)(*dims), (C.c_float * 3)(*vs), (C.c_float * 3)(*org), code)
        cfg = _lib.McConfigC(float(iso_level), (_lib.TC_MC_NORMALS if normals else 0) | (_lib.TC_MC_WELD if weld else 0))
        fn = self._road(v, L.tc_marching_cubes, L.tc_marching_cubes_device)
        nv, nf = C.c_size_t(0), C.c_size_t(0)
        # an empty array (a zero dim) has no address; the library reads no voxel of a grid without cubes, but still makes its checks
        head = (self._h, C.byref(grid), v.ptr or _NO_VOXELS.ctypes.data, (m.ptr or None) if m else None, C.byref(cfg))
        self._check(fn(*head, None, None, None, 0, 0, C.byref(nv), C.byref(nf)))
        out_v, out_f = _new(v.device, (nv.value, 3)), _new(v.device, (nf.value, 3), np.uint32)
        out_n = _new(v.device, (nv.value, 3)) if normals else None
        if nv.value:
            if v.is_torch:
                self._order(v.device)           # the outputs were made on torch's stream
            self._check(fn(*head, _ptr(out_v), None if out_n is None else _ptr(out_n), _ptr(out_f), nv.value, nf.value, C.byref(nv), C.byref(nf)))
        return out_v, out_n, out_f

    # ---- Poisson reconstruction ----
    _POISSON_FIELDS = ("depth", "scale", "point_weight", "max_iterations", "tolerance", "min_density")

    def _poisson_config(self, L, config, overrides):
        """tc_poisson_config from the library's defaults, then `config` (a mapping or an object with some of the fields), then keywords"""
        cfg = _lib.PoissonConfigC()
        L.tc_poisson_config_default(C.byref(cfg))
        given = {} if config is None else (dict(config) if isinstance(config, dict) else {k: getattr(config, k) for k in self._POISSON_FIELDS if hasattr(config, k)})
        given.update({k: v for k, v in overrides.items() if v is not None})
        unknown = set(given) - set(self._POISSON_FIELDS)
        if unknown:
            raise InvalidData(f"poisson: unknown configuration fields {sorted(unknown)}")
        for k, v in given.items():
            if k in ("depth", "max_iterations"):
                if not 0 <= int(v) < 2 ** 32:
                    raise InvalidData(f"poisson: {k} does not fit 32 bits")
                setattr(cfg, k, int(v))
            else:
                setattr(cfg, k, float(v))
        return cfg

    def _poisson_inputs(self, points, normals):
        p = _points(points)
        q = _points(normals, on_device=p.is_torch)
        if q.n != p.n:
            raise InvalidData("poisson: points and normals differ in length")
        if p.is_torch and q.device != p.device:
            raise InvalidData("poisson: normals are not on the points' device")
        return p, q

    @staticmethod
    def _poisson_stats(s):
        return {"iterations": int(s.iterations), "rel_residual": float(s.rel_residual), "iso_value": float(s.iso_value), "occupied_nodes": int(s.occupied_nodes)}

    def poisson_field(self, points, normals, config=None, *, want_chi=True, want_density=True, **overrides):
        """The indicator field of an oriented cloud on a dense grid of 2^depth nodes per axis (tc_poisson_field, the companion library of
        include/threecrate_hip_poisson.h, which states the whole contract and the deviation from the reference's solver).  points,
        normals: (n, 3).  config: a mapping or an object with some of depth, scale, point_weight, max_iterations, tolerance, min_density;
        keywords override it.  numpy arrays take the host entry point, torch device tensors the device one.
        -> {"chi", "density": (N, N, N) float32 indexed [z, y, x] (what marching_cubes takes as layout="x_fastest"), "origin",
        "voxel_size", "dims", and the stats: "iterations", "rel_residual", "iso_value", "occupied_nodes"}."""
        L = _lib.load_companion("threecrate_hip_poisson.h")
        cfg = self._poisson_config(L, config, overrides)
        p, q = self._poisson_inputs(points, normals)
        N = 1 << cfg.depth if _lib.TC_POISSON_MIN_DEPTH <= cfg.depth <= _lib.TC_POISSON_MAX_DEPTH else 1     # (a bad depth fails in the library)
        chi = _new(p.device, (N, N, N)) if want_chi else None
        density = _new(p.device, (N, N, N)) if want_density else None
        grid, stats = _lib.McGridC(), _lib.PoissonStatsC()
        fn = self._road(p, L.tc_poisson_field, L.tc_poisson_field_device)
        self._check(fn(self._h, p.ptr if p.n else None, q.ptr if q.n else None, p.n, C.byref(cfg), C.byref(grid), None if chi is None else _ptr(chi),
                       None if density is None else _ptr(density), C.byref(stats)))
        out = {"chi": chi, "density": density, "origin": tuple(grid.origin), "voxel_size": tuple(grid.voxel_size), "dims": tuple(grid.dims)}
        out.update(self._poisson_stats(stats))
        return out

    def poisson_reconstruct(self, points, normals, config=None, *, return_stats=False, **overrides):
        """poisson_reconstruction (threecrate-reconstruction/src/poisson.rs) over tc_poisson_reconstruct: the field of poisson_field, then
        its welded iso surface at the mean of the field over the points; nodes whose density is below min_density (> 0) are trimmed.
        Two calls: the counts, then the mesh.  -> (vertices (n, 3) f32, faces (m, 3) uint32 (int32 bits for a torch device tensor))
        [, stats].  With outward normals the faces' right-hand normals point inward (the header's step 8)."""
        L = _lib.load_companion("threecrate_hip_poisson.h")
        cfg = self._poisson_config(L, config, overrides)
        p, q = self._poisson_inputs(points, normals)
        fn = self._road(p, L.tc_poisson_reconstruct, L.tc_poisson_reconstruct_device)
        nv, nf, stats = C.c_size_t(0), C.c_size_t(0), _lib.PoissonStatsC()
        head = (self._h, p.ptr if p.n else None, q.ptr if q.n else None, p.n, C.byref(cfg))
        self._check(fn(*head, None, None, 0, 0, C.byref(nv), C.byref(nf), C.byref(stats)))
        out_v, out_f = _new(p.device, (nv.value, 3)), _new(p.device, (nf.value, 3), np.uint32)
        if nv.value and nf.value:
            if p.is_torch:
                self._order(p.device)           # the outputs were made on torch's stream
            self._check(fn(*head, _ptr(out_v), _ptr(out_f), nv.value, nf.value, C.byref(nv), C.byref(nf), C.byref(stats)))
        return (out_v, out_f, self._poisson_stats(stats)) if return_stats else (out_v, out_f)

    # ---- FPFH descriptors ----
    def colorize(self, xyz, sources, *, default_color=(128, 128, 128), interpolation="bilinear", min_depth=1e-4, depth_tolerance=0.05,
                 return_index=False, count=True, return_color=True):
        """Colour a cloud from registered camera images (tc_colorize, the companion library of include/threecrate_hip_color.h): every
        point takes the colour of the first source that sees it, else default_color.  Each source is (image H x W x 3 uint8,
        (fx, fy, cx, cy), world_to_camera 3 x 4 or 4 x 4[, depth H x W float32 metres: the occlusion test]).  numpy arrays take the host
        entry point, torch device tensors the device one; the cloud chooses the road and the images follow it.
        -> colours (n, 3) uint8 [, source index (n,) int32, -1 = none] [, number of coloured points (one read-back)]."""
        L = _lib.load_companion("threecrate_hip_color.h")
        p = _points(xyz)
        mode = {"nearest": _lib.TC_COLOR_NEAREST, "bilinear": _lib.TC_COLOR_BILINEAR}.get(interpolation)
        dc = [int(c) for c in default_color]
        if mode is None or len(dc) != 3 or not all(0 <= c <= 255 for c in dc):
            raise InvalidData('interpolation is "nearest" or "bilinear"; default_color has three entries in 0..255')
        cfg = _lib.ColorizeConfigC((C.c_uint8 * 3)(*dc), mode, float(min_depth), float(depth_tolerance))
        sources = list(sources)
        table, keep = (_lib.ColorSourceC * max(1, len(sources)))(), []
        for s, src in enumerate(sources):
            image, k, m = src[:3]
            shape = tuple(image.shape)
            if len(shape) != 3 or shape[2] != 3 or not 0 <= shape[0] < 2 ** 32 or not 0 <= shape[1] < 2 ** 32:
                raise InvalidData(f"image {s} must have shape (H, W, 3), got {list(shape)}")
            h, w = shape[:2]
            img = _image(image, np.uint8, 3 * h * w, f"image {s}", on_device=p.is_torch)
            dep = None if len(src) < 4 or src[3] is None else _image(src[3], np.float32, h * w, f"depth image {s}", on_device=p.is_torch)
            if any(a is not None and a.device != p.device for a in (img, dep)):
                raise InvalidData(f"image {s} is not on the cloud's device")
            fx, fy, cx, cy = (float(v) for v in k)
            table[s] = _lib.ColorSourceC(img.ptr, dep.ptr if dep else None, _lib.CameraIntrinsicsC(fx, fy, cx, cy, w, h),
                                         (C.c_float * 12)(*TsdfVolume._world_to_camera(None, m)))
            keep += [img, dep]
        rgb = _new(p.device, (p.n, 3), np.uint8) if return_color else None
        idx = _new(p.device, p.n, np.int32) if return_index else None
        n = C.c_size_t(0)
        fn = self._road(p, L.tc_colorize, L.tc_colorize_device)
        self._check(fn(self._h, p.ptr, p.n, table, len(sources), C.byref(cfg), None if rgb is None else _ptr(rgb), None if idx is None else _ptr(idx),
                       C.byref(n) if count else None))
        if p.is_torch and not count:
            self._release(p.device)             # only enqueued: torch may not reuse the cloud or the images before the context's stream has read them
        out = [a for a in (rgb, idx) if a is not None] + ([int(n.value)] if count else [])
        return out[0] if len(out) == 1 else tuple(out)

    def _fpfh(self, cloud, cols, search_radius, k_neighbors, host_fn, dev_fn):
        k = int(k_neighbors)
        if k < 0:
            raise InvalidData("k_neighbors must not be negative")
        x = _points(cloud, cols)
        out = _new(x.device, (x.n, 33), zeros=not x.is_torch)
        self._check(self._road(x, host_fn, dev_fn)(self._h, x.ptr, x.n, float(search_radius), k, _ptr(out)))
        return out

    def extract_fpfh_features_with_normals(self, cloud_n, search_radius: float = 0.1, k_neighbors: int = 10):
        """extract_fpfh_features_with_normals (features.rs:173-259): (n, 6) NormalPoint3f records -> (n, 33) float32, row i the
        descriptor of point i.  Torch device tensors in -> a torch tensor out."""
        L = self._L
        return self._fpfh(cloud_n, 6, search_radius, k_neighbors, L.tc_extract_fpfh_features_with_normals,
                          L.tc_extract_fpfh_features_with_normals_device)

    def extract_fpfh_features(self, cloud, search_radius: float = 0.1, k_neighbors: int = 10):
        """The wheel's extract_fpfh_features (threecrate-python lib.rs:1222-1245): estimate_normals(cloud, k_neighbors), then
        extract_fpfh_features_with_normals with (search_radius, k_neighbors); the normals stay on the device."""
        L = self._L
        return self._fpfh(cloud, 3, search_radius, k_neighbors, L.tc_extract_fpfh_features, L.tc_extract_fpfh_features_device)

    def extract_shot_features(self, normal_points, search_radius: float = 0.2, k_neighbors: int = 10, variant="shot", return_frames=False):
        """extract_shot_features_with_normals (features.rs:591-645; tc_extract_shot_features_with_normals, the companion library of
        include/threecrate_hip_shot.h, which pins the rule and lists the deviations): SHOT (variant "shot", 352 values a row) or USC
        ("usc", 128) descriptors.  normal_points: (n, 6) NormalPoint3f records, or a (cloud (n, 3), normals (n, 3)) pair.  Torch device
        tensors in -> torch tensors out.  return_frames: -> (descriptors, frames (n, 9) float32: x, y, z of every point's local
        reference frame, flags (n,) uint32 (int32 bits for a torch tensor): the road (_lib.TC_SHOT_ROAD_*) and the TC_SHOT_X_TIE,
        TC_SHOT_ZERO_COV and TC_SHOT_EMPTY bits)."""
        L = _lib.load_companion("threecrate_hip_shot.h")
        variants = {"shot": _lib.TC_SHOT_VARIANT_SHOT, "usc": _lib.TC_SHOT_VARIANT_USC}
        if variant not in variants:
            raise InvalidData(f"extract_shot_features: variant is {variant!r}, not 'shot' or 'usc'")
        k = int(k_neighbors)
        if k < 0:
            raise InvalidData("k_neighbors must not be negative")
        if isinstance(normal_points, tuple):
            cloud, normals = normal_points
            if _is_torch(cloud):
                import torch
                normal_points = torch.cat([_f32(cloud, True).reshape(-1, 3), _f32(normals, True).reshape(-1, 3).to(cloud.device)], dim=1)
            else:
                normal_points = np.concatenate([_as_host(cloud, 3), _as_host(normals, 3)], axis=1)
        x = _points(normal_points, 6)
        cfg = _lib.ShotConfigC(float(search_radius), k, variants[variant])
        rows = max(x.n, 1)                                      # (never empty: the library wants a pointer)
        out = _new(x.device, (rows, int(L.tc_shot_dim(cfg.variant))), zeros=not x.is_torch)
        frames = _new(x.device, (rows, 9), zeros=not x.is_torch) if return_frames else None
        flags = _new(x.device, rows, np.uint32, zeros=not x.is_torch) if return_frames else None
        fn = self._road(x, L.tc_extract_shot_features_with_normals, L.tc_extract_shot_features_with_normals_device)
        self._check(fn(self._h, x.ptr if x.n else None, x.n, C.byref(cfg), _ptr(out), None if frames is None else _ptr(frames),
                       None if flags is None else _ptr(flags)))
        return (out[:x.n], frames[:x.n], flags[:x.n]) if return_frames else out[:x.n]

    # ---- ICP ----
    def _result(self, r, ns, corr, want_pairs):
        T = np.array(list(r.transformation), np.float32)
        res = ICPResult(T, float(r.mse), int(r.iterations), bool(r.converged), corr_target=corr)
        if want_pairs is True and corr is not None:
            ct = corr.cpu().numpy() if _is_torch(corr) else corr
            ct = ct.astype(np.int64)
            src = np.nonzero(ct != 0xFFFFFFFF)[0]
            res.correspondences = np.stack([src, ct[src]], axis=1)
        return res

    def icp_detailed(self, source, target, init=None, max_iters=50, max_correspondence_distance=None,
                     convergence_threshold=1e-6, correspondences=True, _checked=False):
        """registration.rs:258-370"""
        md = self._max_dist(max_correspondence_distance)
        i7, r = _init7(init), _lib.IcpResultC()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        corr = _corr_buffer(r, s.device, s.n) if correspondences else None
        if md is None:
            self._reject_all(s.n, t.n, max_iters)
        a, b = md, convergence_threshold
        if s.is_torch:
            # the device entry point has no *_point_to_point twin: its threshold check is made here
            if _checked and not (convergence_threshold > 0):
                raise InvalidData("Convergence threshold must be positive")
            fn = self._L.tc_icp_detailed_device
            self._order(s.device)
        elif _checked:
            fn, a, b = self._L.tc_icp_point_to_point, convergence_threshold, md
        else:
            fn = self._L.tc_icp_detailed
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, max_iters, a, b, C.byref(r)))
        return self._result(r, s.n, _cut_corr(corr, s.n, correspondences), correspondences)

    def gicp(self, source, target, init=None, config: "GicpConfig" = None, correspondences=True):
        """gicp.rs:100-305"""
        cfg = config or GicpConfig()
        c = _lib.GicpConfigC(cfg.max_iterations, cfg.max_correspondence_distance, cfg.convergence_threshold, cfg.k_correspondences)
        i7, r = _init7(init), _lib.IcpResultC()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        corr = _corr_buffer(r, s.device, s.n) if correspondences else None
        fn = self._road(s, self._L.tc_gicp, self._L.tc_gicp_device)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, C.byref(c), C.byref(r)))
        return self._result(r, s.n, _cut_corr(corr, s.n, correspondences), correspondences)

    def kiss_icp(self, source, target, init=None, config: "KissIcpConfig" = None, correspondences=True):
        """kiss_icp.rs:183-300.  `correspondences` pairs (index into the voxel-downsampled source, target index)."""
        cfg = config or KissIcpConfig()
        c = _lib.KissIcpConfigC(cfg.voxel_size, cfg.max_range, cfg.min_range, cfg.max_iterations)
        i7, r, nd = _init7(init), _lib.IcpResultC(), C.c_size_t(0)
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        corr = _corr_buffer(r, s.device, s.n) if correspondences else None
        fn = self._road(s, self._L.tc_kiss_icp, self._L.tc_kiss_icp_device)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, C.byref(c), C.byref(r), C.byref(nd)))
        # (this road has no "device" mode: its pairs index the down-sampled source and always come back masked)
        return self._result(r, nd.value, _cut_corr(corr, nd.value, correspondences, device_bits=False), correspondences)

    def icp_point_to_point(self, source, target, init=None, max_iterations=50, convergence_threshold=1e-6,
                           max_correspondence_distance=None, correspondences=True):
        """registration.rs:644-680 (adds the threshold > 0 check)"""
        return self.icp_detailed(source, target, init, max_iterations, max_correspondence_distance,
                                 convergence_threshold, correspondences, _checked=True)

    def icp(self, source, target, init=None, max_iters=50):
        """registration.rs:232-242: returns the 7-float isometry; any error returns `init`."""
        i7 = _init7(init)
        if _is_torch(source):
            try:
                return self.icp_detailed(source, target, i7, max_iters, None, 1e-6, correspondences=False).transformation
            except Error:
                return i7.copy()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        out = np.zeros(7, np.float32)
        self._check(self._L.tc_icp(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, max_iters, out.ctypes.data))
        return out

    def multiscale_icp_point_to_point(self, source, target, init=None, config=None):
        """registration.rs:704-789"""
        cfg = config or MultiScaleIcpConfig()
        s, t = _points(source, on_device=False), _points(target, on_device=False)      # there is no device entry point
        i7 = _init7(init)
        lv = (_lib.ScaleLevelC * max(1, len(cfg.levels)))()
        for i, l in enumerate(cfg.levels):
            lv[i].voxel_size, lv[i].max_iterations = float(l.voxel_size), int(l.max_iterations)
            lv[i].max_correspondence_distance = self._max_dist_as_given(l.max_correspondence_distance)
        c = _lib.MultiScaleConfigC(lv, len(cfg.levels), int(cfg.final_refinement_iterations),
                                   self._max_dist_as_given(cfg.final_max_correspondence_distance), float(cfg.convergence_threshold))
        r = _lib.IcpResultC()
        corr = _corr_buffer(r, None, s.n)
        self._check(self._L.tc_multiscale_icp_point_to_point(self._h, s.ptr, s.n, t.ptr, t.n, i7.ctypes.data, C.byref(c), C.byref(r)))
        return self._result(r, s.n, _cut_corr(corr, s.n, True), True)

    def icp_point_to_plane_detailed(self, source, target, target_normals, init=None, max_iters=50,
                                    max_correspondence_distance=None, convergence_threshold=1e-6, correspondences=True):
        """registration.rs:508-602.  target_normals: (Nt, 3) Vector3f, or the (Nt, 6) NormalPoint3f
        array returned by estimate_normals (its normal columns are used in place, stride 6)."""
        md = self._max_dist(max_correspondence_distance)
        i7, r = _init7(init), _lib.IcpResultC()
        s = _points(source)
        t = _points(target, on_device=s.is_torch)
        nptr, nn, stride, _keep = _normals_arg(target_normals, on_device=s.is_torch)
        if md is None:
            self._reject_all(s.n, t.n, max_iters, nn)
        corr = _corr_buffer(r, s.device, s.n) if correspondences else None
        fn = self._road(s, self._L.tc_icp_point_to_plane_detailed, self._L.tc_icp_point_to_plane_detailed_device)
        self._check(fn(self._h, s.ptr, s.n, t.ptr, t.n, nptr, nn, stride, i7.ctypes.data, max_iters, md, convergence_threshold, C.byref(r)))
        return self._result(r, s.n, _cut_corr(corr, s.n, correspondences), correspondences)

    def icp_point_to_plane(self, source, target, target_normals, init=None, max_iters=50):
        """registration.rs:488-496"""
        return self.icp_point_to_plane_detailed(source, target, target_normals, init, max_iters, None, 1e-6)


def _hip_memcpy_dtoh(dst, src, nbytes):
    """hipMemcpy(dst, src, nbytes, hipMemcpyDeviceToHost) through the HIP runtime the library is bound to (already in the process'
    global namespace: _lib._preload_hip_runtime / the library's own NEEDED entry) -- never a second copy of the runtime"""
    fn = None
    try:
        fn = C.CDLL(None).hipMemcpy
    except AttributeError:
        # the runtime was loaded without RTLD_GLOBAL (no torch preload: it came in as the library's own NEEDED entry): take the
        # copy that is ALREADY in the process by its soname -- RTLD_NOLOAD never loads a second one
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                fn = C.CDLL(name, mode=os.RTLD_NOLOAD | os.RTLD_NOW).hipMemcpy
                break
            except (OSError, AttributeError):
                continue
    if fn is None:
        return -1
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    fn.restype = C.c_int
    return fn(dst, src, nbytes, 2)


class Cloud(_Handle):
    """Device-resident cloud handle (tc_cloud_*): owns a copy of the points in HBM, is indexed once, keeps its
    normals in the layout the ICP kernels read.  `points`: numpy (uploaded) or a torch CUDA tensor (copied on the device).

        prev = tc.Cloud(ctx, frame0); prev.estimate_normals(16, out=False)
        cur = tc.Cloud(ctx, frame1)
        r = cur.icp_point_to_plane(prev)          # icp_point_to_plane(source=cur, target=prev, prev's normals)
    """

    _destroy = "tc_cloud_destroy"

    def __init__(self, ctx: "GpuContext", points):
        self._ctx, self._L = ctx._track(self), _lib.load()
        h = C.c_void_p()
        x = _points(points)
        if x.is_torch:
            ctx._order(x.device)
            ctx._check(self._L.tc_cloud_upload_device(ctx._h, x.ptr, x.n, C.byref(h)))
            # `x` may be a temporary, or be overwritten by the caller's next torch op: torch's stream waits for the copy (an
            # event, no host wait -- the constructor used to synchronise: 0.1 ms per 1 M-point pair)
            ctx._release(x.device)
        else:
            ctx._check(self._L.tc_cloud_upload(ctx._h, x.ptr, x.n, C.byref(h)))
        self._torch_device = x.device
        self._h = h

    def __len__(self):
        return int(self._L.tc_cloud_size(self._h))

    def estimate_normals(self, k: int = 10, config: "NormalEstimationConfig" = None, out=True):
        """estimate_normals_with_config (normals.rs:257-357) on the handle's cloud; the normals stay with the handle.
        out=True: also return the (n, 6) NormalPoint3f array (torch on the device for a torch-made handle, numpy otherwise);
        out=False: nothing is returned and the scattered 24-byte record stores are skipped."""
        c = self._ctx._cfg(config or NormalEstimationConfig(k_neighbors=k))
        n = len(self)
        if not out:
            self._ctx._check(self._L.tc_cloud_estimate_normals_device(self._h, C.byref(c), None))
            return None
        o = _new(self._torch_device, (n, 6))
        if self._torch_device is not None:
            self._ctx._order(o.device)
            self._ctx._check(self._L.tc_cloud_estimate_normals_device(self._h, C.byref(c), o.data_ptr()))
        else:
            self._ctx._check(self._L.tc_cloud_estimate_normals(self._h, C.byref(c), o.ctypes.data))
        return o

    def normals(self):
        """the handle's (n, 6) NormalPoint3f array in input order (tc_cloud_normals_device; made from the cell-sorted normals on
        demand), as a numpy copy; None when the handle has no normals"""
        p = self._L.tc_cloud_normals_device(self._h)
        if not p:
            return None
        n = len(self)
        self._ctx._check(self._L.tc_synchronize(self._ctx._h))
        host = np.empty((n, 6), np.float32)
        rc = _hip_memcpy_dtoh(host.ctypes.data, p, n * 24)
        if rc != 0:
            raise GpuError(f"hipMemcpy failed ({rc})")
        return host

    def set_normals(self, normals):
        """normals computed elsewhere: (n, 3), or the (n, 6) NormalPoint3f array of an estimate_normals call"""
        if not _is_torch(normals):
            import torch
            normals = torch.from_numpy(_f32(normals)).to(torch.device("cuda", self._ctx.device))
        nptr, nn, stride, t = _normals_arg(normals, on_device=True)
        self._ctx._order(t.device)
        self._ctx._check(self._L.tc_cloud_set_normals_device(self._h, nptr, nn, stride))

    def _icp(self, fn, target, init, max_iters, max_correspondence_distance, convergence_threshold, correspondences, needs_normals):
        import torch
        ctx = self._ctx
        md = ctx._max_dist(max_correspondence_distance)
        if md is None:
            ctx._reject_all(len(self), len(target), max_iters)
        i7, r = _init7(init), _lib.IcpResultC()
        corr = None
        if correspondences:
            corr = _corr_buffer(r, torch.device("cuda", ctx.device), len(self))
            ctx._order(corr.device)
        ctx._check(fn(self._h, target._h, i7.ctypes.data, max_iters, md, convergence_threshold, C.byref(r)))
        if corr is not None:
            corr = _cut_corr(corr, len(self), correspondences)
        return ctx._result(r, len(self), corr, correspondences)

    def icp_point_to_plane(self, target: "Cloud", init=None, max_iters=50, max_correspondence_distance=None,
                           convergence_threshold=1e-6, correspondences=False):
        """icp_point_to_plane_detailed (registration.rs:508-602): self = source, `target` = a handle with normals"""
        return self._icp(self._L.tc_cloud_icp_point_to_plane, target, init, max_iters, max_correspondence_distance, convergence_threshold,
                         correspondences, True)

    def icp_detailed(self, target: "Cloud", init=None, max_iters=50, max_correspondence_distance=None, convergence_threshold=1e-6,
                     correspondences=False):
        """icp_detailed (registration.rs:258-370): self = source"""
        return self._icp(self._L.tc_cloud_icp_detailed, target, init, max_iters, max_correspondence_distance, convergence_threshold,
                         correspondences, False)


# ---- module-level free functions with the reference's names ----------------------------------
_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = GpuContext(0)
    return _default_ctx


def estimate_normals(cloud, k=10, ctx=None):
    return (ctx or default_context()).estimate_normals(cloud, k)


def estimate_normals_with_config(cloud, config, ctx=None):
    return (ctx or default_context()).estimate_normals_with_config(cloud, config)


def estimate_normals_radius(cloud, radius, consistent_orientation, ctx=None):
    return (ctx or default_context()).estimate_normals_radius(cloud, radius, consistent_orientation)


def voxel_grid_filter(cloud, voxel_size, ctx=None):
    return (ctx or default_context()).voxel_grid_filter(cloud, voxel_size)


def gpu_voxel_grid_filter(gpu_context, cloud, voxel_size):
    """threecrate-gpu/src/lib.rs:50 facade name; semantics of the CPU voxel_grid_filter (centroids)."""
    return gpu_context.voxel_grid_filter(cloud, voxel_size)


def extract_euclidean_clusters(cloud, tolerance, min_cluster_size, max_cluster_size, ctx=None):
    return (ctx or default_context()).extract_euclidean_clusters(cloud, tolerance, min_cluster_size, max_cluster_size)


def gpu_extract_euclidean_clusters(gpu_context, cloud, tolerance, min_cluster_size, max_cluster_size):
    """threecrate-gpu/src/segmentation.rs:473-645 facade name; exact (no max_neighbors cap), partition on the device."""
    return gpu_context.extract_euclidean_clusters(cloud, tolerance, min_cluster_size, max_cluster_size)


def extract_fpfh_features_with_normals(cloud_n, search_radius=0.1, k_neighbors=10, ctx=None):
    return (ctx or default_context()).extract_fpfh_features_with_normals(cloud_n, search_radius, k_neighbors)


def extract_fpfh_features(cloud, search_radius=0.1, k_neighbors=10, ctx=None):
    return (ctx or default_context()).extract_fpfh_features(cloud, search_radius, k_neighbors)


def statistical_outlier_removal(cloud, k_neighbors, std_dev_multiplier, return_index=False, return_mean_distance=False, ctx=None):
    return (ctx or default_context()).statistical_outlier_removal(cloud, k_neighbors, std_dev_multiplier, return_index, return_mean_distance)


def statistical_outlier_removal_with_threshold(cloud, k_neighbors, threshold, return_index=False, return_mean_distance=False, ctx=None):
    return (ctx or default_context()).statistical_outlier_removal_with_threshold(cloud, k_neighbors, threshold, return_index,
                                                                               return_mean_distance)


def radius_outlier_removal(cloud, radius, min_neighbors, return_index=False, ctx=None):
    return (ctx or default_context()).radius_outlier_removal(cloud, radius, min_neighbors, return_index)


def gpu_remove_statistical_outliers(gpu_context, cloud, k_neighbors, std_dev_multiplier):
    """gpu_remove_statistical_outliers (threecrate-gpu/src/filtering.rs:882-893)"""
    return gpu_context.statistical_outlier_removal(cloud, k_neighbors, std_dev_multiplier)


def gpu_radius_outlier_removal(gpu_context, cloud, radius, min_neighbors):
    """gpu_radius_outlier_removal (threecrate-gpu/src/filtering.rs:895-905)"""
    return gpu_context.radius_outlier_removal(cloud, radius, min_neighbors)


def segment_plane(cloud, threshold, max_iters, seed=0, ctx=None):
    """segment_plane(&cloud, threshold, max_iters) (segmentation.rs:117-180) -> PlaneSegmentationResult"""
    return (ctx or default_context()).segment_plane(cloud, threshold, max_iters, seed)


def segment_plane_ransac(cloud, max_iters, threshold, ctx=None):
    """segment_plane_ransac(&cloud, max_iters, threshold) (segmentation.rs:297-304; note the argument order) -> (coefficients, inliers)"""
    r = (ctx or default_context()).segment_plane(cloud, threshold, max_iters)
    return r.plane_coefficients, r.inlier_indices


def plane_segmentation_ransac(cloud, max_iters, threshold, ctx=None):
    """plane_segmentation_ransac (segmentation.rs:318-324): an alias of segment_plane_ransac"""
    return segment_plane_ransac(cloud, max_iters, threshold, ctx)


def gpu_segment_plane_ransac(gpu_context, cloud, threshold, max_iters):
    """gpu_segment_plane_ransac (threecrate-gpu/src/segmentation.rs:822-831) -> PlaneSegmentationResult.  Unlike the facade, equal
    scores go to the lowest iteration and the score divides by the normal's length (include/threecrate_hip_segmentation.h)."""
    return gpu_context.segment_plane(cloud, threshold, max_iters)


def gpu_segment_plane(gpu_context, cloud, config=None):
    """gpu_segment_plane (threecrate-gpu/src/segmentation.rs:304-324, :813-819): config.min_inliers == 0 is InvalidData after the
    checks of the inputs (:853-861), a winner with fewer inliers than config.min_inliers an AlgorithmError."""
    config = config or GpuPlaneSegmentationConfig()
    if int(config.min_inliers) == 0:
        n = _points(cloud).n
        if n >= 3 and not config.distance_threshold <= 0.0 and int(config.max_iterations) != 0:
            raise InvalidData("min_inliers must be at least 1")
    r = gpu_context.segment_plane(cloud, config.distance_threshold, config.max_iterations)
    if r.num_inliers < int(config.min_inliers):
        raise AlgorithmError(f"Plane model has {r.num_inliers} inliers, below required minimum {int(config.min_inliers)}")
    return r


def create_tsdf_volume(voxel_size, truncation_distance, resolution, origin=(0, 0, 0), max_weight=100, ctx=None):
    """create_tsdf_volume (tsdf.rs:806-818) -> TsdfVolume on `ctx`"""
    return (ctx or default_context()).tsdf_volume(voxel_size, truncation_distance, resolution, origin, max_weight)


def gpu_tsdf_integrate(gpu_context, volume, depth_image, color_image, camera_pose, intrinsics):
    """gpu_tsdf_integrate (tsdf.rs:821-832): fuses into `volume` and returns its voxels (tsdf, weight, rgb) as the reference does --
    the download is the call shape's price; TsdfVolume.integrate leaves the state on the device.  `volume` is the persistent handle:
    frames ACCUMULATE across calls, where the reference (and the Rust facade's function of this name) starts from a fresh volume every
    time -- volume.reset() first gives that meaning."""
    volume.integrate(depth_image, intrinsics, camera_pose=camera_pose, color=color_image)
    return volume.voxels()


def gpu_tsdf_extract_surface(gpu_context, volume, voxels, iso_value):
    """gpu_tsdf_extract_surface (tsdf.rs:835-844): `voxels` = (tsdf, weight[, rgb]) is loaded into `volume` first (None: the
    volume's own state) -> (xyz, rgb)"""
    if voxels is not None:
        volume.load(*voxels)
    return volume.extract_surface(iso_value)


def global_registration(source, target, config=None, ctx=None):
    """global_registration (global_registration.rs:185-201)"""
    return (ctx or default_context()).global_registration(source, target, config)


def global_registration_with_normals(source_n, target_n, source, target, config=None, ctx=None):
    """global_registration_with_normals (global_registration.rs:213-333): source_n / target_n are (n, 6) NormalPoint3f records"""
    return (ctx or default_context()).global_registration(source, target, config, source_n, target_n)


def ndt_registration(source, target, init=None, config=None, ctx=None):
    """ndt_registration(&source, &target, initial_transform, &config) (ndt_registration.rs:188-260) -> NdtResult"""
    c = config or NdtConfig()
    return (ctx or default_context()).ndt_registration(source, target, init, c.resolution, c.step_size, c.max_iterations, c.epsilon,
                                                       c.min_points_per_voxel)


def ndt_registration_default(source, target, init=None, ctx=None):
    """ndt_registration_default (ndt_registration.rs:263-269)"""
    return ndt_registration(source, target, init, NdtConfig(), ctx)


def icp(source, target, init=None, max_iters=50, ctx=None):
    return (ctx or default_context()).icp(source, target, init, max_iters)


def icp_detailed(source, target, init, max_iters, max_correspondence_distance=None, convergence_threshold=1e-6, ctx=None):
    return (ctx or default_context()).icp_detailed(source, target, init, max_iters, max_correspondence_distance,
                                                   convergence_threshold)


def icp_point_to_point(source, target, init, max_iterations, convergence_threshold=1e-6,
                       max_correspondence_distance=None, ctx=None):
    return (ctx or default_context()).icp_point_to_point(source, target, init, max_iterations, convergence_threshold,
                                                         max_correspondence_distance)


def gicp(source, target, init, config=None, ctx=None):
    """gicp.rs:100-105"""
    return (ctx or default_context()).gicp(source, target, init, config)


def kiss_icp(source, target, init, config=None, ctx=None):
    """kiss_icp.rs:183-188"""
    return (ctx or default_context()).kiss_icp(source, target, init, config)


def icp_point_to_point_default(source, target, init, max_iterations, ctx=None):
    """registration.rs:694-701"""
    return icp_point_to_point(source, target, init, max_iterations, 1e-6, None, ctx)


def icp_point_to_plane(source, target, target_normals, init, max_iters, ctx=None):
    return (ctx or default_context()).icp_point_to_plane(source, target, target_normals, init, max_iters)


def icp_point_to_plane_detailed(source, target, target_normals, init, max_iters, max_correspondence_distance=None,
                                convergence_threshold=1e-6, ctx=None):
    return (ctx or default_context()).icp_point_to_plane_detailed(source, target, target_normals, init, max_iters,
                                                                  max_correspondence_distance, convergence_threshold)


# ---- threecrate-gpu facade (threecrate-gpu/src/lib.rs:48-60) ---------------------------------
def gpu_estimate_normals(gpu_context, cloud, k):
    """threecrate-gpu/src/normals.rs:443-461"""
    return gpu_context.estimate_normals(cloud, k)


def gpu_icp(gpu_context, source, target, max_iterations, convergence_threshold, max_correspondence_distance):
    """threecrate-gpu/src/icp.rs:977-994 -> Isometry3 (7 floats); starts from identity (:202)."""
    return gpu_context.icp_point_to_point(source, target, None, max_iterations, convergence_threshold,
                                          max_correspondence_distance, correspondences=False).transformation


def gpu_icp_point_to_plane(gpu_context, source, target, target_normals, max_iterations, convergence_threshold,
                           max_correspondence_distance):
    """threecrate-gpu/src/icp.rs:1017-1036"""
    return gpu_context.icp_point_to_plane_detailed(source, target, target_normals, None, max_iterations,
                                                   max_correspondence_distance, convergence_threshold, correspondences=False)


@dataclass
class BatchICPJob:
    """threecrate-gpu/src/icp.rs:132-139"""
    source: np.ndarray
    target: np.ndarray
    max_iterations: int
    convergence_threshold: float
    max_correspondence_distance: float


@dataclass
class BatchICPResult:
    """threecrate-gpu/src/icp.rs:142-147 (+ per-job status)"""
    transformation: np.ndarray
    final_error: float
    iterations: int
    status: int = 0


def gpu_batch_icp(gpu_contexts, jobs):
    """threecrate-gpu/src/icp.rs:997-1002; job i runs on gpu_contexts[i % len]; contexts on
    different GPUs run concurrently."""
    ctxs = gpu_contexts if isinstance(gpu_contexts, (list, tuple)) else [gpu_contexts]
    L = _lib.load()
    arr = (C.c_void_p * len(ctxs))(*[c._h for c in ctxs])
    keep = []
    cj = (_lib.BatchJobC * max(1, len(jobs)))()
    for i, j in enumerate(jobs):
        s, t = _as_host(j.source), _as_host(j.target)
        keep += [s, t]
        cj[i].source, cj[i].n_source, cj[i].target, cj[i].n_target = s.ctypes.data, s.shape[0], t.ctypes.data, t.shape[0]
        cj[i].max_iterations = j.max_iterations
        cj[i].convergence_threshold = j.convergence_threshold
        cj[i].max_correspondence_distance = j.max_correspondence_distance
    cr = (_lib.BatchResultC * max(1, len(jobs)))()
    rc = L.tc_batch_icp(arr, len(ctxs), cj, len(jobs), cr)
    if rc != _lib.TC_OK:
        raise InvalidData("tc_batch_icp: bad arguments")
    return [BatchICPResult(np.array(list(cr[i].transformation), np.float32), float(cr[i].final_error),
                           int(cr[i].iterations), int(cr[i].status)) for i in range(len(jobs))]


# ---- LiDAR frame streaming (RealtimePipeline, threecrate-algorithms/src/streaming.rs:540-646) -------
@dataclass
class BackpressureConfig:
    """streaming.rs BackpressureConfig: only max_queue_depth applies to whole-frame items."""
    max_queue_depth: int = 4


@dataclass
class FrameResult:
    transformation: np.ndarray      # current frame -> previous frame (7-float Isometry3)
    mse: float
    iterations: int
    converged: bool
    status: int
    n_points_in: int
    n_points: int

    @property
    def matrix(self):
        return isometry_to_matrix(self.transformation)


@dataclass
class RealtimeMetrics:
    items_queued: int
    items_processed: int
    items_dropped: int
    max_depth_seen: int


class FrameStream(_Handle):
    """Bounded-queue frame registration pipeline on one GPU (tc_frame_stream_*): send() blocks when the
    queue is full, try_send() drops instead, finish() drains and returns (results, metrics).  Frames are
    host arrays (n, 3) or KITTI records (n, 4)."""

    _destroy = "tc_frame_stream_destroy"

    def __init__(self, ctx: "GpuContext", max_points: int, voxel_size: float = 0.2, k_neighbors: int = 16,
                 max_iterations: int = 50, max_correspondence_distance=None, convergence_threshold: float = 1e-6,
                 backpressure: BackpressureConfig = None):
        self._ctx, self._L = ctx._track(self), _lib.load()
        bp = backpressure or BackpressureConfig()
        cfg = _lib.FrameStreamConfigC(max_points, bp.max_queue_depth, voxel_size, k_neighbors, max_iterations,
                                      GpuContext._max_dist_as_given(max_correspondence_distance),
                                      convergence_threshold)
        h = C.c_void_p()
        ctx._check(self._L.tc_frame_stream_create(ctx._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self._sent = 0

    def _frame(self, frame):
        a = np.ascontiguousarray(np.asarray(frame, np.float32))
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise InvalidData("a frame is an (n, 3) xyz or (n, 4) KITTI x, y, z, intensity array")
        return a

    def send(self, frame):
        a = self._frame(frame)
        self._ctx._check(self._L.tc_frame_stream_send(self._h, a.ctypes.data, a.shape[0], a.shape[1]))
        self._sent += 1

    def try_send(self, frame) -> bool:
        a = self._frame(frame)
        ok = C.c_int(0)
        self._ctx._check(self._L.tc_frame_stream_try_send(self._h, a.ctypes.data, a.shape[0], a.shape[1], C.byref(ok)))
        self._sent += int(ok.value)
        return bool(ok.value)

    def finish(self):
        cap = max(self._sent, 1)
        res = (_lib.FrameResultC * cap)()
        n = C.c_size_t(0)
        m = _lib.FrameStreamMetricsC()
        rc = self._L.tc_frame_stream_finish(self._h, res, cap, C.byref(n), C.byref(m))
        self.close()
        self._ctx._check(rc)
        out = [FrameResult(np.array(list(r.transformation), np.float32), float(r.mse), int(r.iterations), bool(r.converged),
                           int(r.status), int(r.n_points_in), int(r.n_points)) for r in res[:min(n.value, cap)]]
        return out, RealtimeMetrics(int(m.items_queued), int(m.items_processed), int(m.items_dropped), int(m.max_depth_seen))


class SearchIndex(_Handle):
    """Persistent neighbour-search object (tc_search_index_*): KdTree::new once (nearest_neighbor.rs:37-58), then
    find_k_nearest / find_radius_neighbors (core/traits.rs:6-12) for any number of queries against the same cloud.
    The cloud (numpy or torch-on-device) is copied, cell-sorted, into device memory owned by the handle."""

    _destroy = "tc_search_index_destroy"

    def __init__(self, ctx: "GpuContext", cloud, k_hint: int = 16):
        self._ctx, self._L = ctx._track(self), _lib.load()
        h = C.c_void_p()
        x = _points(cloud)
        fn = ctx._road(x, self._L.tc_search_index_create, self._L.tc_search_index_create_device)
        ctx._check(fn(ctx._h, x.ptr, x.n, int(k_hint), C.byref(h)))
        self._h = h

    def __len__(self):
        return int(self._L.tc_search_index_size(self._h))

    def _query(self, queries, k, radius):
        q = _points(queries)
        idx, dist, cnt = _search_out(q.device, q.n, k)
        fn = self._ctx._road(q, self._L.tc_search_index_query, self._L.tc_search_index_query_device)
        self._ctx._check(fn(self._h, q.ptr, q.n, int(k), float(radius), _ptr(idx), _ptr(dist), _ptr(cnt)))
        return (idx, dist, cnt) if q.is_torch else (idx.astype(np.int64), dist, cnt)

    def find_k_nearest_batch(self, queries, k: int):
        """(idx (nq, k), dist (nq, k), count (nq,)); rows ascending by distance, entries past count[q] undefined"""
        return self._query(queries, k, -1.0)

    def find_radius_neighbors_batch(self, queries, radius: float, k_max: int = 32):
        """the neighbours within radius among the k_max nearest; count[q] == k_max: there may be more.  A radius that is not
        positive (0, negative, NaN) has no neighbours (nearest_neighbor.rs:255-259): it goes to the library as 0, never as the
        negative or NaN that tc_search_index_query reads as "the k nearest"."""
        radius = float(radius)
        return self._query(queries, k_max, radius if radius > 0.0 else 0.0)

    def radius_counts(self, queries, radius: float):
        """number of cloud points within `radius` of every host query (tc_search_index_radius_count)"""
        q = _as_host(queries)
        cnt = np.zeros(len(q), np.uint32)
        self._ctx._check(self._L.tc_search_index_radius_count(self._h, q.ctypes.data, q.shape[0], float(radius), cnt.ctypes.data))
        return cnt

    def find_radius_neighbors_all(self, queries, radius: float):
        """NearestNeighborSearch::find_radius_neighbors (nearest_neighbor.rs:254-298) for many host queries, WITHOUT a cap:
        (offsets (nq + 1,) int64, idx (total,) int64, dist (total,) f32); query q owns [offsets[q], offsets[q + 1]),
        ascending by distance like the reference's final sort."""
        q = _as_host(queries)
        cnt = np.zeros(len(q), np.uint32)
        self._ctx._check(self._L.tc_search_index_radius_count(self._h, q.ctypes.data, q.shape[0], float(radius), cnt.ctypes.data))
        off = np.zeros(len(q) + 1, np.uint64)
        np.cumsum(cnt, out=off[1:])
        total = int(off[-1])
        idx, dist = np.zeros(total, np.uint32), np.zeros(total, np.float32)
        if total:
            self._ctx._check(self._L.tc_search_index_radius_fill(self._h, q.ctypes.data, q.shape[0], float(radius), off.ctypes.data, total,
                                                                 idx.ctypes.data, dist.ctypes.data))
            seg = np.repeat(np.arange(len(q)), cnt.astype(np.int64))
            order = np.lexsort((idx, dist, seg))            # per query: by distance, ties by index
            idx, dist = idx[order], dist[order]
        return off.astype(np.int64), idx.astype(np.int64), dist

    def find_k_nearest(self, query, k: int):
        return _first_row(*self.find_k_nearest_batch(_one_query(query), k))

    def find_radius_neighbors(self, query, radius: float, k_max: int = 32):
        return _first_row(*self.find_radius_neighbors_batch(_one_query(query), radius, k_max))


class _image:
    """an image as the TSDF entry points take it: contiguous, of `dtype`, of the depth image's kind (`on_device`), with the size the
    intrinsics state"""
    __slots__ = ("a", "ptr", "device")

    def __init__(self, a, dtype, numel, what, on_device=None):
        if _is_torch(a) if on_device is None else on_device:
            import torch
            self.a = a.detach().to(getattr(torch, np.dtype(dtype).name)).contiguous()
            self.device, size = self.a.device, self.a.numel()
        else:
            self.a, self.device = np.ascontiguousarray(np.asarray(a, dtype=dtype)), None
            size = self.a.size
        if size != numel:
            raise InvalidData(f"{what} has {size} values, the intrinsics ask for {numel}")
        self.ptr = _ptr(self.a)

    @property
    def is_torch(self):
        return self.device is not None


class TsdfVolume(_Handle):
    """A dense TSDF volume that lives in device memory (tc_tsdf_volume_*): integrate() fuses a depth image into it in place,
    extract_surface() reads it in place.  Arrays are in voxel index order, x fastest: shaped (rz, ry, rx[, 3])."""

    _destroy = "tc_tsdf_volume_destroy"

    def __init__(self, ctx: "GpuContext", voxel_size, truncation_distance, resolution, origin=(0, 0, 0), max_weight=100):
        self._ctx, self._L = ctx._track(self), _lib.load()
        res, org, mw = [int(r) for r in resolution], [float(o) for o in origin], int(max_weight)
        if len(res) != 3 or len(org) != 3 or min(res) < 0 or not 0 <= mw < 2 ** 32 or max(res) >= 2 ** 32:
            raise InvalidData("resolution and origin have three entries; resolution and max_weight must not be negative")
        cfg = _lib.TsdfVolumeConfigC(float(voxel_size), float(truncation_distance), (C.c_uint32 * 3)(*res), (C.c_float * 3)(*org), mw)
        h = C.c_void_p()
        ctx._check(self._L.tc_tsdf_volume_create(ctx._h, C.byref(cfg), C.byref(h)))
        self._h = h
        self.voxel_size, self.truncation_distance, self.resolution, self.origin, self.max_weight = cfg.voxel_size, cfg.truncation_distance, tuple(res), tuple(org), mw
        self.n_voxels = res[0] * res[1] * res[2]

    @staticmethod
    def _world_to_camera(camera_pose, world_to_camera):
        if (camera_pose is None) == (world_to_camera is None):
            if camera_pose is not None:
                raise InvalidData("give camera_pose or world_to_camera, not both")
            return np.ascontiguousarray(np.eye(4, dtype=np.float32)[:3].reshape(12))
        if world_to_camera is not None:
            m = np.asarray(world_to_camera, np.float32)
            return np.ascontiguousarray((m.reshape(4, 4)[:3] if m.size == 16 else m).reshape(12))
        try:                # float64, then one rounding: tsdf.rs:105-109, with its error
            inv = np.linalg.inv(np.asarray(camera_pose, np.float64).reshape(4, 4))
        except np.linalg.LinAlgError:
            raise GpuError("Failed to invert camera pose matrix") from None
        return np.ascontiguousarray(inv[:3].astype(np.float32).reshape(12))

    def integrate(self, depth, intrinsics: "CameraIntrinsics", camera_pose=None, color=None, world_to_camera=None, count=False):
        """Fuse one depth image (H x W, metres) and optionally its colours (H x W x 3 uint8).  camera_pose: camera-to-world 4 x 4,
        inverted here; or world_to_camera: the 3 x 4 (or 4 x 4) matrix the kernel multiplies by, as it is.  numpy images take the host
        entry point, torch device tensors the device one; the depth image chooses the road.  count=True returns the number of voxels
        updated (one read-back), else None."""
        k = _lib.CameraIntrinsicsC(float(intrinsics.fx), float(intrinsics.fy), float(intrinsics.cx), float(intrinsics.cy), int(intrinsics.width),
                                   int(intrinsics.height))
        m = self._world_to_camera(camera_pose, world_to_camera)
        d = _image(depth, np.float32, k.width * k.height, "the depth image")
        c = None if color is None else _image(color, np.uint8, 3 * k.width * k.height, "the colour image", on_device=d.is_torch)
        n = C.c_size_t(0)
        fn = self._ctx._road(d, self._L.tc_tsdf_integrate, self._L.tc_tsdf_integrate_device)
        self._ctx._check(fn(self._h, d.ptr, c.ptr if c else None, C.byref(k), m.ctypes.data_as(C.POINTER(C.c_float)), C.byref(n) if count else None))
        if d.is_torch and not count:
            self._ctx._release(d.device)        # only enqueued: torch may not reuse the images before the context's stream has read them
        return int(n.value) if count else None

    def reset(self):
        """back to the initial state: tsdf 1.0, weight 0, colour (0, 0, 0)"""
        self._ctx._check(self._L.tc_tsdf_volume_reset(self._h))

    def voxels(self):
        """(tsdf (rz, ry, rx) f32, weight (rz, ry, rx) u8, rgb (rz, ry, rx, 3) u8) on the host (download_voxels, tsdf.rs:739-792)"""
        rx, ry, rz = self.resolution
        tsdf, weight, rgb = np.empty((rz, ry, rx), np.float32), np.empty((rz, ry, rx), np.uint8), np.empty((rz, ry, rx, 3), np.uint8)
        self._ctx._check(self._L.tc_tsdf_volume_download(self._h, _ptr(tsdf), _ptr(weight), _ptr(rgb)))
        return tsdf, weight, rgb

    def load(self, tsdf, weight, rgb=None):
        """set the state from arrays in voxel index order (any shape of the right size); the tsdf array chooses the road"""
        t = _image(tsdf, np.float32, self.n_voxels, "tsdf")
        w = _image(weight, np.uint8, self.n_voxels, "weight", on_device=t.is_torch)
        c = None if rgb is None else _image(rgb, np.uint8, 3 * self.n_voxels, "rgb", on_device=t.is_torch)
        fn = self._ctx._road(t, self._L.tc_tsdf_volume_upload, self._L.tc_tsdf_volume_upload_device)
        self._ctx._check(fn(self._h, t.ptr, w.ptr, c.ptr if c else None))

    def extract_surface(self, iso_value=0.0, observed_only=False, device=None):
        """-> (xyz (n, 3) f32, rgb (n, 3) u8): the points of surface_extraction.wgsl in a fixed order, without its cap.
        observed_only: an edge needs weight > 0 at both ends (TC_TSDF_OBSERVED_EDGES).  device: a torch device for the outputs (the
        device entry point), numpy otherwise.  Two calls: the count, then the points."""
        flags = _lib.TC_TSDF_OBSERVED_EDGES if observed_only else 0
        fn = self._L.tc_tsdf_extract_surface if device is None else self._L.tc_tsdf_extract_surface_device
        n = C.c_size_t(0)
        self._ctx._check(fn(self._h, float(iso_value), flags, None, None, 0, C.byref(n)))
        xyz, rgb = _new(device, (n.value, 3)), _new(device, (n.value, 3), np.uint8)
        if n.value:
            if device is not None:
                self._ctx._order(xyz.device)
            self._ctx._check(fn(self._h, float(iso_value), flags, _ptr(xyz), _ptr(rgb), n.value, C.byref(n)))
        return xyz, rgb


    def extract_mesh(self, iso_value=0.0, weld=True, normals=False, device=None):
        """The volume's iso surface as a triangle mesh (marching cubes, include/threecrate_hip_mc.h): the state is copied into device
        tensors (tc_tsdf_volume_download_device) and meshed there in the volume's own x-fastest order, with valid = weight > 0 (the
        weight array as it is), so unobserved space gives no triangles.  weld=True: one vertex per grid edge, what smooth_mesh and
        simplify_mesh_clustering take.  device: a torch device for the outputs; None: the mesh comes back as numpy arrays.
        Per-vertex colour is out of scope.  -> (vertices, normals or None, faces) as GpuContext.marching_cubes gives them."""
        import torch
        dev = torch.device("cuda", self._ctx.device) if device is None else torch.device(device)
        rx, ry, rz = self.resolution
        tsdf, weight = _new(dev, (rz, ry, rx)), _new(dev, (rz, ry, rx), np.uint8)
        self._ctx._order(dev)
        self._ctx._check(self._L.tc_tsdf_volume_download_device(self._h, _ptr(tsdf), _ptr(weight), None))
        v, n, f = self._ctx.marching_cubes(tsdf, (rx, ry, rz), self.voxel_size, self.origin, iso_value, normals, weld, weight, "x_fastest")
        if device is None:
            v, f = v.cpu().numpy(), f.cpu().numpy().view(np.uint32)
            n = None if n is None else n.cpu().numpy()
        return v, n, f


class VoxelMap(_Handle):
    """A voxel map that lives in device memory across the chunks of a point stream (tc_voxel_map_*, the companion library of
    include/threecrate_hip_voxelmap.h): insert() folds a chunk into it, extract() reads it without changing it.  The state after a
    stream does not depend on how the stream was cut into chunks."""

    _destroy = "tc_voxel_map_destroy"

    def __init__(self, ctx: "GpuContext", voxel_size, initial_capacity=0):
        self._ctx, self._L = ctx._track(self), _lib.load_companion("threecrate_hip_voxelmap.h")
        cap = int(initial_capacity)
        if not 0 <= cap < 2 ** 64:
            raise InvalidData("initial_capacity must not be negative")
        cfg = _lib.VoxelMapConfigC(float(voxel_size), cap)
        h = C.c_void_p()
        rc = self._L.tc_voxel_map_create(ctx._h, C.byref(cfg), C.byref(h))
        ctx._check(rc)
        self._h = h
        self.voxel_size = cfg.voxel_size

    def insert(self, points):
        """the next chunk of the stream: (n, 3) float32, numpy (the host entry point) or a torch device tensor (the device one)"""
        p = _points(points)
        fn = self._ctx._road(p, self._L.tc_voxel_map_insert, self._L.tc_voxel_map_insert_device)
        self._ctx._check(fn(self._h, p.ptr, p.n))
        if p.is_torch:
            self._ctx._release(p.device)        # only enqueued: torch may not reuse the chunk before the context's stream has read it

    def __len__(self):
        return int(self._L.tc_voxel_map_size(self._h))

    @property
    def points_inserted(self):
        return int(self._L.tc_voxel_map_points(self._h))

    def reset(self):
        """no voxels, no points; the table keeps its size"""
        self._ctx._check(self._L.tc_voxel_map_reset(self._h))

    def extract(self, keys=False, counts=False, sums=False, device=None):
        """-> centroids (V, 3) f32 in ascending (kx, ky, kz) order, followed by what was asked for: keys (V, 3) int32, counts (V,)
        uint32, sums (V, 3) float64.  device: a torch device for the outputs (the device entry point), numpy otherwise.  Two calls:
        the count, then the arrays."""
        fn = self._L.tc_voxel_map_extract if device is None else self._L.tc_voxel_map_extract_device
        n = C.c_size_t(0)
        self._ctx._check(fn(self._h, None, None, None, None, 0, C.byref(n)))
        v = n.value
        if device is None:
            out = [np.empty((v, 3), np.float32), np.empty((v, 3), np.int32) if keys else None, np.empty(v, np.uint32) if counts else None,
                   np.empty((v, 3), np.float64) if sums else None]
        else:
            import torch
            out = [torch.empty((v, 3), dtype=torch.float32, device=device), torch.empty((v, 3), dtype=torch.int32, device=device) if keys else None,
                   torch.empty(v, dtype=torch.int32, device=device) if counts else None,
                   torch.empty((v, 3), dtype=torch.float64, device=device) if sums else None]
        if v:
            if device is not None:
                self._ctx._order(out[0].device)
            ptr = [None if a is None else _ptr(a) for a in out]
            self._ctx._check(fn(self._h, ptr[1], ptr[2], ptr[3], ptr[0], v, C.byref(n)))
        got = [a for a in out if a is not None]
        return got[0] if len(got) == 1 else tuple(got)


def read_kitti_bin(path):
    """VelodyneKittiBinReader::read (threecrate-io/src/lidar.rs:310-343) -> (n, 3) float32."""
    L = _lib.load()
    n = C.c_size_t(0)
    p = os.fsencode(path)
    rc = L.tc_read_kitti_bin(p, None, 0, C.byref(n))
    if rc != _lib.TC_OK:
        raise InvalidData(f"Velodyne KITTI binary: cannot read {path} or its size is not a multiple of 16 bytes")
    out = np.empty((n.value, 3), np.float32)
    if n.value:
        rc = L.tc_read_kitti_bin(p, out.ctypes.data, n.value, C.byref(n))
        if rc != _lib.TC_OK:
            raise InvalidData(f"Velodyne KITTI binary: cannot read {path}")
    return out
