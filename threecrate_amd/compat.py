"""`import threecrate_amd.compat as threecrate` -- the call shapes of the reference's Python module
(threecrate-python/src/lib.rs, stubs threecrate-python/threecrate.pyi) for the functions of this backend's path,
served by the HIP library.  Same class and function names, argument names, defaults, return shapes and exception
types (`RuntimeError` for algorithm / data errors like `to_py_err` lib.rs:40-42, `ValueError` for malformed arrays
lib.rs:85-128,~150-200, `IndexError` from `PointCloud.__getitem__`).

Covered: PointCloud, NormalPointCloud, IcpResult, KdTree, voxel_downsample, remove_statistical_outliers,
remove_radius_outliers, estimate_normals, icp,
icp_point_to_plane, gicp, kiss_icp, concatenate, transform_point_cloud, extract_clusters,
extract_fpfh_features, segment_plane, PlaneSegmentationResult, ndt_registration, NdtResult, global_registration,
global_registration_with_normals, GlobalRegistrationResult, RealtimeVoxelFilter, RealtimeMetrics, ColoredPointCloud,
colorize_point_cloud, TriangleMesh, smooth_mesh_laplacian, smooth_mesh_taubin, smooth_mesh_hc, ClusteringSimplifier,
QuadricErrorSimplifier, alpha_shape_reconstruct, estimate_optimal_alpha, PatchworkConfig, GroundSegmentationResult,
patchwork_plus_plus, segment_ground, ShotConfig, ShotVariant, extract_shot_features_with_normals (the library's names: the wheel has no
SHOT function), PoissonConfig, poisson_reconstruct, poisson_reconstruct_with_normals.  Everything else of that
module (the other mesh operations, the other reconstructions, I/O formats, ROS messages) is outside SURVEY.md section 8.
"""
import numpy as np

from . import api as _api

__all__ = ["PointCloud", "NormalPointCloud", "IcpResult", "KdTree", "voxel_downsample", "remove_statistical_outliers",
           "remove_radius_outliers", "estimate_normals", "icp",
           "icp_point_to_plane", "gicp", "kiss_icp", "concatenate", "transform_point_cloud", "extract_clusters",
           "extract_fpfh_features", "segment_plane", "PlaneSegmentationResult", "ndt_registration", "NdtResult",
           "global_registration", "global_registration_with_normals", "GlobalRegistrationResult", "RealtimeVoxelFilter", "RealtimeMetrics",
           "ColoredPointCloud", "colorize_point_cloud", "TriangleMesh", "smooth_mesh_laplacian", "smooth_mesh_taubin", "smooth_mesh_hc",
           "ClusteringSimplifier", "QuadricErrorSimplifier", "alpha_shape_reconstruct", "estimate_optimal_alpha",
           "PatchworkConfig", "GroundSegmentationResult", "patchwork_plus_plus", "segment_ground",
           "ShotConfig", "ShotVariant", "extract_shot_features_with_normals",
           "PoissonConfig", "poisson_reconstruct", "poisson_reconstruct_with_normals"]


def _nx3(arr, what="Array"):
    """read_nx3_points (lib.rs): (N, 3) float32 or float64 -> float32"""
    if not isinstance(arr, np.ndarray) or arr.dtype not in (np.float32, np.float64):
        raise ValueError("Expected a numpy array of shape (N, 3) with dtype float32 or float64")
    if arr.ndim != 2 or arr.shape[1] != 3:
        raise ValueError(f"{what} must have shape (N, 3), got shape {list(arr.shape)} with dtype {arr.dtype}")
    return np.ascontiguousarray(arr, np.float32)


def _run(fn, *a, **k):
    try:
        return fn(*a, **k)
    except _api.Error as e:            # InvalidData / AlgorithmError / GpuError / Unsupported
        raise RuntimeError(str(e)) from None


def _isometry(mat):
    """numpy_to_isometry (lib.rs:76-137): 4 x 4 float32 / float64 -> (qi qj qk qw tx ty tz); None -> identity.
    The rotation is the closest rotation to the upper-left 3 x 3 block (what UnitQuaternion::from_matrix iterates
    to), here by polar decomposition in f64."""
    if mat is None:
        return None
    if not isinstance(mat, np.ndarray) or mat.dtype not in (np.float32, np.float64):
        raise ValueError("init_transform must be a 4×4 numpy array (float32 or float64)")
    if mat.shape != (4, 4):
        raise ValueError("init_transform must be a 4×4 array")
    m = mat.astype(np.float32).astype(np.float64)
    u, _, vt = np.linalg.svd(m[:3, :3])
    r = u @ np.diag([1.0, 1.0, np.sign(np.linalg.det(u @ vt)) or 1.0]) @ vt
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
    q = np.array([i, j, k, w]) / np.sqrt(i * i + j * j + k * k + w * w)
    return np.concatenate([q, m[:3, 3]]).astype(np.float32)


class PointCloud:
    """A 3D point cloud holding XYZ positions (lib.rs PyPointCloud)."""

    def __init__(self, arr=None):
        self._p = np.zeros((0, 3), np.float32) if arr is None else _nx3(arr)

    @staticmethod
    def from_numpy(arr):
        return PointCloud(arr)

    def to_numpy(self):
        return self._p.copy()

    @property
    def points(self):
        return self.to_numpy()

    @property
    def is_empty(self):
        return len(self._p) == 0

    def __len__(self):
        return len(self._p)

    def __getitem__(self, idx):
        n = len(self._p)
        i = n + idx if idx < 0 else idx
        if i < 0 or i >= n:
            raise IndexError("point cloud index out of range")
        return self._p[i].copy()

    def __add__(self, other):
        return PointCloud(np.concatenate([self._p, other._p]))

    def __array__(self, dtype=None, copy=None):
        a = self.to_numpy()
        return a if dtype is None else a.astype(dtype)

    def __repr__(self):
        return f"PointCloud({len(self._p)} points)"


class NormalPointCloud:
    """Positions + normals; returned by estimate_normals, accepted by icp_point_to_plane (lib.rs PyNormalPointCloud)."""

    def __init__(self, _pn=None):
        self._pn = np.zeros((0, 6), np.float32) if _pn is None else _pn

    @staticmethod
    def from_numpy(positions, normals):
        p, n = _nx3(positions, "Positions array"), _nx3(normals, "Normals array")
        if len(p) != len(n):
            raise ValueError(f"positions and normals must have the same length, got {len(p)} and {len(n)}")
        return NormalPointCloud(np.ascontiguousarray(np.concatenate([p, n], axis=1)))

    @property
    def is_empty(self):
        return len(self._pn) == 0

    def positions(self):
        return self._pn[:, 0:3].copy()

    def normals(self):
        return self._pn[:, 3:6].copy()

    def __len__(self):
        return len(self._pn)

    def __repr__(self):
        return f"NormalPointCloud({len(self._pn)} points)"


class ColoredPointCloud:
    """Positions + RGB colours; returned by colorize_point_cloud (lib.rs PyColoredPointCloud)."""

    def __init__(self, _p=None, _c=None):
        self._p = np.zeros((0, 3), np.float32) if _p is None else _p
        self._c = np.zeros((0, 3), np.uint8) if _c is None else _c

    @staticmethod
    def from_numpy(positions, colors):
        p = _nx3(positions)
        if not isinstance(colors, np.ndarray) or colors.dtype != np.uint8 or colors.ndim != 2:
            raise ValueError("colors must be a (N, 3) uint8 numpy array")
        if colors.shape[1] != 3:
            raise ValueError(f"colors must have shape (N, 3), got {list(colors.shape)}")
        if len(p) != len(colors):
            raise ValueError(f"positions and colors must have the same length ({len(p)} vs {len(colors)})")
        return ColoredPointCloud(p, np.ascontiguousarray(colors))

    @property
    def is_empty(self):
        return len(self._p) == 0

    def positions(self):
        return self._p.copy()

    def colors(self):
        return self._c.copy()

    def __len__(self):
        return len(self._p)

    def __repr__(self):
        return f"ColoredPointCloud({len(self._p)} points)"


def _mx3_faces(arr):
    """read_mx3_faces (lib.rs:204-231): (M, 3) uint32, int32, uint64 or int64 -> uint32.  The wheel casts `as usize`: a negative or too
    large index is out of range for every mesh, and stays so here (0xFFFFFFFF)."""
    if not isinstance(arr, np.ndarray) or arr.ndim != 2 or arr.dtype not in (np.uint32, np.int32, np.uint64, np.int64):
        raise ValueError("Faces array must be (M, 3) integer numpy array (int32, int64, uint32, or uint64)")
    if arr.shape[1] != 3:
        raise ValueError(f"Faces array must have shape (M, 3), got {list(arr.shape)}")
    if arr.dtype == np.uint32:
        return np.ascontiguousarray(arr)
    bad = (arr < 0) | (arr > 0xFFFFFFFF) if arr.dtype != np.uint64 else arr > np.uint64(0xFFFFFFFF)
    return np.where(bad, 0xFFFFFFFF, arr).astype(np.uint32)


class TriangleMesh:
    """Vertices + triangular faces (lib.rs PyTriangleMesh)."""

    def __init__(self):
        self._v = np.zeros((0, 3), np.float32)
        self._f = np.zeros((0, 3), np.uint32)

    @staticmethod
    def from_numpy(vertices, faces):
        mesh = TriangleMesh()
        mesh._v, mesh._f = _nx3(vertices), _mx3_faces(faces)
        return mesh

    @property
    def vertex_count(self):
        return len(self._v)

    @property
    def face_count(self):
        return len(self._f)

    @property
    def is_empty(self):
        return len(self._v) == 0

    def vertices(self):
        return self._v.copy()

    def faces(self):
        return self._f.copy()

    def __repr__(self):
        return f"TriangleMesh({len(self._v)} vertices, {len(self._f)} faces)"


class IcpResult:
    """lib.rs:519-547"""

    def __init__(self, r):
        self._m = r.matrix
        self.mse = float(r.mse)
        self.iterations = int(r.iterations)
        self.converged = bool(r.converged)

    def transformation(self):
        """4 x 4 float32 rigid transform (source -> target)"""
        return self._m.copy()

    def __repr__(self):
        return f"IcpResult(converged={'true' if self.converged else 'false'}, mse={self.mse:.6f}, iterations={self.iterations})"


class NdtResult:
    """lib.rs:595-633"""

    def __init__(self, r):
        self._m = r.matrix
        self.score = float(r.score)
        self.iterations = int(r.iterations)
        self.converged = bool(r.converged)

    def transformation(self):
        """4 x 4 float32 rigid transform (source -> target)"""
        return self._m.copy()

    def __repr__(self):
        return f"NdtResult(converged={'true' if self.converged else 'false'}, score={self.score:.6f}, iterations={self.iterations})"


def _query3(query):
    if not isinstance(query, np.ndarray) or query.dtype not in (np.float32, np.float64) or query.ndim != 1:
        raise ValueError("Query point must be a 1D numpy array (float32 or float64)")
    if query.shape[0] != 3:
        raise ValueError("Query point must be a 1D array of length 3")
    return query.astype(np.float32)


class KdTree:
    """Spatial index over a cloud (lib.rs:707-776): built once (a device-resident grid index, tc_search_index_*), then
    queried; results as KdTree::find_k_nearest / find_radius_neighbors (nearest_neighbor.rs:177-298), radius results
    nearest first."""

    def __init__(self, cloud):
        self._n = len(cloud)                 # an empty cloud gives an empty tree (nearest_neighbor.rs:38-45)
        self._ix = _run(_api.SearchIndex, _api.default_context(), cloud._p)

    def knn(self, query, k):
        q = _query3(query)
        if k == 0 or self._n == 0:           # nearest_neighbor.rs:178-180
            return [], []
        pairs = _run(self._ix.find_k_nearest, q, min(int(k), self._n))
        return [i for i, _ in pairs], [d for _, d in pairs]

    def radius_search(self, query, radius):
        q = _query3(query)
        if self._n == 0:
            return [], []
        _, idx, dist = _run(self._ix.find_radius_neighbors_all, q.reshape(1, 3), float(radius))
        return [int(i) for i in idx], [float(d) for d in dist]

    def __repr__(self):
        return "KdTree"


def voxel_downsample(cloud, voxel_size):
    """voxel_grid_filter (filtering.rs:38-133); voxels come out sorted by (kx, ky, kz)"""
    return PointCloud(np.asarray(_run(_api.default_context().voxel_grid_filter, cloud._p, float(voxel_size)), np.float32))


def estimate_normals(cloud, k_neighbors=10):
    """lib.rs:827-833 -> estimate_normals (normals.rs:238-241)"""
    return NormalPointCloud(np.ascontiguousarray(_run(_api.default_context().estimate_normals, cloud._p, int(k_neighbors)), np.float32))


def icp(source, target, max_iterations=50, init_transform=None):
    """lib.rs:850-862 -> icp_point_to_point_default (registration.rs:683-701: threshold 1e-6, no distance limit)"""
    init = _isometry(init_transform)
    return IcpResult(_run(_api.default_context().icp_point_to_point, source._p, target._p, init, int(max_iterations), 1e-6, None,
                          correspondences=False))


def icp_point_to_plane(source, target, max_iterations=50, init_transform=None):
    """lib.rs:963-1007 -> icp_point_to_plane (registration.rs:488-494)"""
    init = _isometry(init_transform)
    return IcpResult(_run(_api.default_context().icp_point_to_plane, source._p, np.ascontiguousarray(target._pn[:, 0:3]),
                          np.ascontiguousarray(target._pn[:, 3:6]), init, int(max_iterations)))


def gicp(source, target, max_iterations=50, max_correspondence_distance=1.0, convergence_threshold=1e-6, k_correspondences=20,
         init_transform=None):
    """lib.rs:878-906 -> gicp (gicp.rs:100-305)"""
    init = _isometry(init_transform)
    cfg = _api.GicpConfig(int(max_iterations), float(max_correspondence_distance), float(convergence_threshold), int(k_correspondences))
    return IcpResult(_run(_api.default_context().gicp, source._p, target._p, init, cfg))


def kiss_icp(source, target, voxel_size=1.0, max_range=100.0, min_range=0.5, max_iterations=50, init_transform=None):
    """lib.rs:922-950 -> kiss_icp (kiss_icp.rs:183-300)"""
    init = _isometry(init_transform)
    cfg = _api.KissIcpConfig(float(voxel_size), float(max_range), float(min_range), int(max_iterations))
    return IcpResult(_run(_api.default_context().kiss_icp, source._p, target._p, init, cfg))


def ndt_registration(source, target, init_transform=None, resolution=1.0, step_size=0.1, max_iterations=35, epsilon=1e-4,
                     min_points_per_voxel=5):
    """lib.rs:1165-1201 -> ndt_registration (ndt_registration.rs:188-260)"""
    init = _isometry(init_transform)
    return NdtResult(_run(_api.default_context().ndt_registration, source._p, target._p, init, float(resolution), float(step_size),
                          int(max_iterations), float(epsilon), int(min_points_per_voxel)))


def colorize_point_cloud(cloud, image_data, width, height, fx, fy, cx, cy, world_to_camera):
    """lib.rs:1595-1613: one registered RGB image (raw bytes, row-major R G B), the default configuration (grey (128, 128, 128) for
    points no pixel colours, bilinear, min_depth 1e-4) -> ColoredPointCloud"""
    data = np.frombuffer(image_data, np.uint8)
    width, height = int(width), int(height)
    expected = width * height * 3
    if data.size < expected:                    # RgbImageView::new, colorization.rs:60-70
        raise RuntimeError(f"RgbImageView: buffer too small — expected {expected} bytes for {width}×{height} RGB image, got {data.size}")
    if world_to_camera is None:
        raise ValueError("init_transform must be a 4×4 numpy array (float32 or float64)")
    pose = _api.isometry_to_matrix(_isometry(world_to_camera))
    rgb = _run(_api.default_context().colorize, cloud._p, [(data[:expected].reshape(height, width, 3), (fx, fy, cx, cy), pose)], count=False)
    return ColoredPointCloud(cloud._p.copy(), rgb)


def _smooth_mesh(mesh, method, iterations, **params):
    if len(mesh._v) == 0 or len(mesh._f) == 0:          # TriangleMesh::is_empty (mesh_smoothing.rs:99-101), before the parameters
        raise RuntimeError("Mesh is empty")
    if int(iterations) < 0:
        raise OverflowError("can't convert negative int to unsigned")
    out = TriangleMesh()
    out._v, out._f = _run(_api.default_context().smooth_mesh, mesh._v, mesh._f, method, int(iterations), **params), mesh._f.copy()
    return out


def smooth_mesh_laplacian(mesh, iterations=10, lambda_=0.5):
    """lib.rs:1405-1419: `iterations` Laplacian steps with lambda_ in (0, 1] -> a new TriangleMesh with the same faces"""
    return _smooth_mesh(mesh, "laplacian", iterations, lambda_=lambda_)


def smooth_mesh_taubin(mesh, iterations=10, lambda_=0.5, mu=-0.53):
    """lib.rs:1433-1450: per iteration a step with lambda_ in (0, 1) and a step with mu < 0"""
    return _smooth_mesh(mesh, "taubin", iterations, lambda_=lambda_, mu=mu)


def smooth_mesh_hc(mesh, iterations=10, alpha=0.0, beta=0.5):
    """lib.rs:1461-1478: HC (Humphrey's Classes) smoothing, alpha and beta in [0, 1]"""
    return _smooth_mesh(mesh, "hc", iterations, alpha=alpha, beta=beta)


class ClusteringSimplifier:
    """ClusteringSimplifier (threecrate-simplification/src/clustering.rs:495-506, the fields of with_params) with
    .simplify(mesh, reduction_ratio) -> TriangleMesh, its uniform road on the device.  mode="adaptive" (a sequential octree) and
    representative_strategy="minimum_error" (nalgebra's matrix inverse) raise Unsupported.  The quadric road is QuadricErrorSimplifier,
    below; the wheel's function name for it, `simplify_mesh`, joins this module once the test that holds it absent
    (tests/test_simplify_cpu.py::test_python_surface) may change."""

    def __init__(self, mode="uniform", representative_strategy="centroid", preserve_boundary=True,
                 feature_angle_threshold=_api.GpuContext.SIMPLIFY_DEFAULT_FEATURE_ANGLE):
        if mode != "uniform":
            raise _api.Unsupported(f"ClusteringSimplifier: mode {mode!r} is not supported by the HIP backend (uniform only)")
        if representative_strategy == "minimum_error":
            raise _api.Unsupported("ClusteringSimplifier: the minimum-error representative is not supported by the HIP backend")
        self.mode, self.representative_strategy = mode, representative_strategy
        self.preserve_boundary, self.feature_angle_threshold = bool(preserve_boundary), float(feature_angle_threshold)

    def simplify(self, mesh, reduction_ratio):
        if len(mesh._v) == 0 or len(mesh._f) == 0:          # TriangleMesh::is_empty (clustering.rs:786-788), before the ratio
            raise RuntimeError("Mesh is empty")
        out = TriangleMesh()
        out._v, out._f = _run(_api.default_context().simplify_mesh_clustering, mesh._v, mesh._f, float(reduction_ratio), self.representative_strategy,
                              self.preserve_boundary, self.feature_angle_threshold)
        return out


class QuadricErrorSimplifier:
    """QuadricErrorSimplifier (threecrate-simplification/src/quadric_error.rs:66-100, the fields of with_params) with
    .simplify(mesh, reduction_ratio) -> TriangleMesh: quadric-error edge collapse in rounds on the device (include/threecrate_hip_qem.h),
    what the wheel's simplify_mesh(mesh, reduction_ratio) runs with the defaults.  feature_angle_threshold is accepted, stored and
    IGNORED: quadric_error.rs never reads the field either."""

    def __init__(self, max_edge_length=None, preserve_boundary=True, feature_angle_threshold=_api.GpuContext.SIMPLIFY_DEFAULT_FEATURE_ANGLE):
        self.max_edge_length = None if max_edge_length is None else float(max_edge_length)
        self.preserve_boundary, self.feature_angle_threshold = bool(preserve_boundary), float(feature_angle_threshold)

    def simplify(self, mesh, reduction_ratio):
        if len(mesh._v) == 0 or len(mesh._f) == 0:          # TriangleMesh::is_empty (quadric_error.rs:414-416), before the ratio
            raise RuntimeError("Mesh is empty")
        out = TriangleMesh()
        out._v, out._f = _run(_api.default_context().simplify_mesh_quadric, mesh._v, mesh._f, float(reduction_ratio), self.preserve_boundary,
                              self.max_edge_length)
        return out


def alpha_shape_reconstruct(cloud, alpha=1.0):
    """alpha_shape_reconstruct (lib.rs:1533-1537; alpha_shape_reconstruction, alpha_shape.rs): the boundary triangles of the alpha complex
    over the cloud's own points, with the reference's cap of 50 000 candidates in index order (include/threecrate_hip_alpha.h; for the
    whole cloud: GpuContext.alpha_shape(..., max_triangles=0)).  "No candidate triangles generated" and "No triangles survived alpha
    filtering" are RuntimeError, like every Error of the wheel."""
    if len(cloud._p) == 0:                                  # alpha_shape.rs:125-127
        raise RuntimeError("Point cloud is empty")
    mesh = TriangleMesh()
    mesh._f = _run(_api.default_context().alpha_shape, cloud._p, float(alpha))
    mesh._v = cloud._p.copy()
    return mesh


def estimate_optimal_alpha(cloud, k):
    """estimate_optimal_alpha (alpha_shape.rs:543-583): every step-th point is a sample, step = max(n / clamp(n / 10, 50, 500), 1); a
    sample's value is the distance to its k-th nearest OTHER point, entry k of the (k + 1)-list of the batch k-NN export, which holds the
    sample itself at distance 0; the median by [len / 2], times 1.8f.  1.0 when no sample has k other points."""
    pts = cloud._p
    n, k = len(pts), int(k)
    if n == 0:
        raise RuntimeError("Point cloud is empty")
    if k < 1:
        raise RuntimeError("estimate_optimal_alpha: k must be at least 1")
    if n - 1 < k:
        return 1.0
    step = max(n // min(max(n // 10, 50), 500), 1)
    _, dist, _ = _run(_api.default_context().find_k_nearest_batch, pts, pts[::step], k + 1)
    kth = np.sort(dist[:, k].astype(np.float32))
    return float(kth[len(kth) // 2] * np.float32(1.8))


class PatchworkConfig:
    """PatchworkConfig (ground_segmentation.rs:24-77): the reference's field names and defaults, lists for the per-zone fields"""

    def __init__(self, sensor_height=1.723, zone_radii=(0.0, 2.7, 12.3625, 22.025, 80.0), num_rings_per_zone=(2, 4, 4, 4),
                 num_sectors_per_zone=(16, 32, 54, 32), max_range=80.0, min_points_per_patch=10, num_seed_points=20,
                 seed_selection_threshold=0.5, dist_threshold=0.125, num_iterations=3, uprightness_threshold=0.707, flatness_threshold=0.05,
                 elevation_threshold=1.0):
        self.sensor_height = float(sensor_height)
        self.zone_radii, self.num_rings_per_zone = list(zone_radii), list(num_rings_per_zone)
        self.num_sectors_per_zone = list(num_sectors_per_zone)
        self.max_range, self.min_points_per_patch, self.num_seed_points = float(max_range), int(min_points_per_patch), int(num_seed_points)
        self.seed_selection_threshold, self.dist_threshold = float(seed_selection_threshold), float(dist_threshold)
        self.num_iterations, self.uprightness_threshold = int(num_iterations), float(uprightness_threshold)
        self.flatness_threshold, self.elevation_threshold = float(flatness_threshold), float(elevation_threshold)

    def _c(self):
        return _api.GpuContext.ground_config(
            self.sensor_height, zone_radii=self.zone_radii, num_rings=self.num_rings_per_zone, num_sectors=self.num_sectors_per_zone,
            max_range=self.max_range, min_points_per_patch=self.min_points_per_patch, num_seed_points=self.num_seed_points,
            seed_selection_threshold=self.seed_selection_threshold, dist_threshold=self.dist_threshold, num_iterations=self.num_iterations,
            uprightness_threshold=self.uprightness_threshold, flatness_threshold=self.flatness_threshold,
            elevation_threshold=self.elevation_threshold)


class GroundSegmentationResult:
    """GroundSegmentationResult (ground_segmentation.rs:81-88): the two clouds and a label per input point"""

    def __init__(self, ground, nonground, labels):
        self.ground, self.nonground, self.labels = ground, nonground, labels

    def __repr__(self):
        return f"GroundSegmentationResult(ground={len(self.ground)}, nonground={len(self.nonground)})"


def patchwork_plus_plus(cloud, config=None):
    """patchwork_plus_plus (ground_segmentation.rs:336-407) over include/threecrate_hip_ground.h, which lists the deviations (f64 sums; a
    point that is not finite is non-ground)."""
    config = PatchworkConfig() if config is None else config
    r = _run(lambda: _api.default_context().segment_ground(cloud._p, config=config._c(), return_points=True, return_patches=False))
    return GroundSegmentationResult(PointCloud(np.ascontiguousarray(r["ground_points"])), PointCloud(np.ascontiguousarray(r["nonground_points"])),
                                    [bool(b) for b in r["labels"]])


def segment_ground(cloud, sensor_height):
    """segment_ground (ground_segmentation.rs:410-419): the default configuration with the given sensor height"""
    return patchwork_plus_plus(cloud, PatchworkConfig(sensor_height=sensor_height))


class VolumetricGrid:
    """VolumetricGrid (threecrate-reconstruction/src/marching_cubes.rs:12-65): `values` shaped (nx, ny, nz), zeros at first"""

    def __init__(self, dimensions, voxel_size, origin):
        self.dimensions = tuple(int(d) for d in dimensions)
        self.voxel_size = tuple(float(np.float32(v)) for v in voxel_size)
        self.origin = tuple(float(np.float32(o)) for o in origin)
        if len(self.dimensions) != 3 or len(self.voxel_size) != 3 or len(self.origin) != 3 or min(self.dimensions) < 0:
            raise _api.InvalidData("dimensions, voxel_size and origin have three entries")
        self.values = np.zeros(self.dimensions, np.float32)

    def _inside(self, x, y, z):
        return 0 <= x < self.dimensions[0] and 0 <= y < self.dimensions[1] and 0 <= z < self.dimensions[2]

    def get_value(self, x, y, z):
        """the value, or None outside the grid"""
        return float(self.values[x, y, z]) if self._inside(x, y, z) else None

    def set_value(self, x, y, z, value):
        if not self._inside(x, y, z):
            raise _api.InvalidData(f"Grid coordinates ({x}, {y}, {z}) out of bounds for dimensions {list(self.dimensions)}")
        self.values[x, y, z] = value

    def grid_to_world(self, x, y, z):
        """origin + f32(i) * voxel_size per axis, in f32"""
        o, v = np.asarray(self.origin, np.float32), np.asarray(self.voxel_size, np.float32)
        return o + np.asarray([x, y, z], np.float32) * v


class MarchingCubesConfig:
    """MarchingCubesConfig and its default (marching_cubes.rs:141-161)"""

    def __init__(self, iso_level=0.0, compute_normals=True, smooth_mesh=False, smoothing_iterations=3):
        self.iso_level, self.compute_normals = float(iso_level), bool(compute_normals)
        self.smooth_mesh, self.smoothing_iterations = bool(smooth_mesh), int(smoothing_iterations)


class MarchingCubes:
    """MarchingCubes::new(config).extract_isosurface(grid) -> TriangleMesh, unwelded like the reference (a vertex per crossing edge per
    cube); the normals, when computed, are kept as `mesh.normals`.  The per-cube triangulation comes from this project's generated case
    table, not the reference's (include/threecrate_hip_mc.h).  smooth_mesh=True raises Unsupported: the reference's neighbour sum runs
    in hash-set order, which cannot be pinned; smooth_mesh_laplacian smooths a welded mesh."""

    def __init__(self, config=None):
        self.config = config if config is not None else MarchingCubesConfig()

    def extract_isosurface(self, grid):
        c = self.config
        if c.smooth_mesh:
            raise _api.Unsupported("MarchingCubes: smooth_mesh is not supported by the HIP backend")
        values = np.ascontiguousarray(grid.values, np.float32)
        if values.shape != tuple(grid.dimensions):
            raise _api.InvalidData("VolumetricGrid: values must be shaped like dimensions")
        if min(grid.dimensions) < 2:            # no cubes
            raise _api.AlgorithmError("No isosurface found at specified level")
        v, n, f = _api.default_context().marching_cubes(values, grid.dimensions, grid.voxel_size, grid.origin, c.iso_level, c.compute_normals, False)
        if len(v) == 0:
            raise _api.AlgorithmError("No isosurface found at specified level")
        mesh = TriangleMesh()
        mesh._v, mesh._f, mesh.normals = v, f, n
        return mesh


def marching_cubes(grid, iso_level):
    """marching_cubes(grid, iso_level) (marching_cubes.rs:857-864): the default config with this level"""
    return MarchingCubes(MarchingCubesConfig(iso_level=iso_level)).extract_isosurface(grid)


def concatenate(clouds):
    """lib.rs:1633-1642"""
    return PointCloud(np.concatenate([c._p for c in clouds]) if len(clouds) else np.zeros((0, 3), np.float32))


def transform_point_cloud(cloud, transform):
    """lib.rs:1660-1675: every point through the Isometry3 built from the 4 x 4 (quaternion form, f32)"""
    iso = _isometry(transform)
    if iso is None:
        raise ValueError("init_transform must be a 4×4 numpy array (float32 or float64)")
    q, t = iso[:4].astype(np.float32), iso[4:7].astype(np.float32)
    p = cloud._p
    qv = q[:3]
    t2 = np.cross(np.broadcast_to(qv, p.shape), p).astype(np.float32) * np.float32(2.0)
    out = ((t2 * q[3] + np.cross(np.broadcast_to(qv, p.shape), t2).astype(np.float32)) + p) + t
    return PointCloud(out.astype(np.float32))


def remove_statistical_outliers(cloud, k_neighbors=20, std_ratio=2.0):
    """lib.rs:789-803 -> statistical_outlier_removal (filtering.rs:249-321): the kept points in input order"""
    return PointCloud(_run(_api.default_context().statistical_outlier_removal, cloud._p, int(k_neighbors), float(std_ratio)))


def remove_radius_outliers(cloud, radius, min_neighbors):
    """lib.rs:805-817 -> radius_outlier_removal (filtering.rs:167-213): the kept points in input order"""
    return PointCloud(_run(_api.default_context().radius_outlier_removal, cloud._p, float(radius), int(min_neighbors)))


class PlaneSegmentationResult:
    """lib.rs:636-690: the fitted plane and the indices of its inliers"""

    def __init__(self, coefficients, inliers):
        self._c, self._inliers = np.asarray(coefficients, np.float32), inliers

    def plane_coefficients(self):
        """(4,) float32: a, b, c, d of a*x + b*y + c*z + d = 0; (a, b, c) is the unit normal"""
        return self._c.copy()

    def inlier_indices(self):
        """indices of the inlier points in the original cloud (sorted)"""
        return [int(i) for i in self._inliers]

    @property
    def num_inliers(self):
        return len(self._inliers)

    def inlier_cloud(self, cloud):
        return PointCloud(np.ascontiguousarray(cloud._p[self._inliers.astype(np.int64)]))

    def __repr__(self):
        return f"PlaneSegmentationResult(inliers={len(self._inliers)}, normal=[{self._c[0]:.3f}, {self._c[1]:.3f}, {self._c[2]:.3f}])"


def segment_plane(cloud, threshold=0.01, max_iterations=1000):
    """lib.rs:1251-1277 -> segment_plane (segmentation.rs:117-180).  The wheel draws its triples from the thread's RNG; here they
    come from the GPU facade's deterministic generator, so the same call returns the same plane."""
    r = _run(_api.default_context().segment_plane, cloud._p, float(threshold), int(max_iterations))
    return PlaneSegmentationResult(r.plane_coefficients, r.inlier_indices)


def extract_clusters(cloud, tolerance=0.02, min_cluster_size=100, max_cluster_size=25000):
    """lib.rs:1294-1316 -> extract_euclidean_clusters (segmentation.rs:396-455): one PointCloud per cluster, largest first;
    the points of a cluster in ascending original index (the CPU path lists them in BFS order: the same sets)"""
    clusters = _run(_api.default_context().extract_euclidean_clusters, cloud._p, float(tolerance), int(min_cluster_size),
                    int(max_cluster_size))
    return [PointCloud(cloud._p[idx]) for idx in clusters]


def extract_fpfh_features(cloud, search_radius=0.1, k_neighbors=10):
    """lib.rs:1222-1245 -> estimate_normals(cloud, k_neighbors), then extract_fpfh_features_with_normals (features.rs:173-259):
    an (N, 33) float32 array, row i the descriptor of point i"""
    return np.ascontiguousarray(_run(_api.default_context().extract_fpfh_features, cloud._p, float(search_radius), int(k_neighbors)),
                                np.float32)


class GlobalRegistrationResult:
    """lib.rs:566-592: the coarse (or refined) pose with RANSAC's inlier statistics"""

    def __init__(self, r):
        self._t = np.ascontiguousarray(r.matrix, np.float32)
        self.inlier_count, self.inlier_ratio = int(r.inlier_count), float(r.inlier_ratio)
        self.icp_mse = None if r.icp_result is None else float(r.icp_result.mse)
        self.icp_converged = None if r.icp_result is None else bool(r.icp_result.converged)

    def transformation(self):
        """the 4 x 4 rigid transformation (source -> target), float32"""
        return self._t.copy()

    def __repr__(self):
        return f"GlobalRegistrationResult(inliers={self.inlier_count}, ratio={self.inlier_ratio:.3f})"


def _global_config(ransac_iterations, distance_threshold, inlier_ratio, fpfh_radius, fpfh_k_neighbors, normal_k_neighbors, refine_with_icp,
                   icp_max_iterations):
    return _api.GlobalRegistrationConfig(int(ransac_iterations), float(distance_threshold), float(inlier_ratio), float(fpfh_radius),
                                         int(fpfh_k_neighbors), int(normal_k_neighbors), bool(refine_with_icp), int(icp_max_iterations), None)


def global_registration(source, target, ransac_iterations=50_000, distance_threshold=0.05, inlier_ratio=0.25, fpfh_radius=0.25,
                        fpfh_k_neighbors=10, normal_k_neighbors=10, refine_with_icp=True, icp_max_iterations=50):
    """lib.rs:1038-1076 -> global_registration (global_registration.rs:185-201).  The wheel draws its RANSAC samples from the thread's
    RNG; here they come from a seeded generator on the device, so the same call returns the same pose."""
    cfg = _global_config(ransac_iterations, distance_threshold, inlier_ratio, fpfh_radius, fpfh_k_neighbors, normal_k_neighbors,
                         refine_with_icp, icp_max_iterations)
    return GlobalRegistrationResult(_run(_api.default_context().global_registration, source._p, target._p, cfg))


def global_registration_with_normals(source_normals, target_normals, source, target, ransac_iterations=50_000, distance_threshold=0.05,
                                     inlier_ratio=0.25, fpfh_radius=0.25, fpfh_k_neighbors=10, normal_k_neighbors=10, refine_with_icp=True,
                                     icp_max_iterations=50):
    """lib.rs:1101-1147 -> global_registration_with_normals (global_registration.rs:213-333)"""
    cfg = _global_config(ransac_iterations, distance_threshold, inlier_ratio, fpfh_radius, fpfh_k_neighbors, normal_k_neighbors,
                         refine_with_icp, icp_max_iterations)
    return GlobalRegistrationResult(_run(_api.default_context().global_registration, source._p, target._p, cfg, source_normals._pn,
                                         target_normals._pn))


def _point3(arr):
    """numpy1d_to_point (lib.rs:140-164)"""
    if not isinstance(arr, np.ndarray) or arr.ndim != 1 or arr.dtype not in (np.float32, np.float64):
        raise ValueError("Query point must be a 1D float numpy array of length 3 (float32 or float64)")
    if arr.shape[0] != 3:
        raise ValueError("Query point must be a 1D array of length 3")
    return arr.astype(np.float32).reshape(1, 3)


class RealtimeMetrics:
    """PyRealtimeMetrics: a snapshot of the pipeline's counters"""

    def __init__(self, queued, processed, dropped):
        self.items_queued, self.items_processed, self.items_dropped = queued, processed, dropped
        self.estimated_queue_depth = queued - processed - dropped

    def __repr__(self):
        return (f"RealtimeMetrics(queued={self.items_queued}, processed={self.items_processed}, dropped={self.items_dropped}, "
                f"depth={self.estimated_queue_depth})")


class RealtimeVoxelFilter:
    """lib.rs:2380-2497 on the device-resident voxel map (GpuContext.voxel_map).  The wheel hands the points to a worker thread in
    chunks of chunk_size; here they are buffered on the host and inserted in batches of this class's own size, on the calling thread:
    the map's state does not depend on how the stream is cut into chunks, so the result is the same.  Nothing is ever dropped:
    try_send always returns True.  max_queue_depth, chunk_size and flush_timeout_ms are checked as the wheel checks them and
    otherwise unused.  The output order is the map's (ascending voxel key), where the wheel's is its HashMap's."""

    _BATCH = 1 << 16        # points per insert

    def __init__(self, voxel_size, max_queue_depth=1024, chunk_size=256, flush_timeout_ms=10):
        if np.float32(voxel_size) <= 0.0:
            raise ValueError("voxel_size must be positive")
        if int(chunk_size) == 0:
            raise ValueError("chunk_size must be ≥ 1")
        if int(max_queue_depth) == 0:
            raise ValueError("max_queue_depth must be ≥ 1")
        self._voxel_size, self._map, self._open = float(voxel_size), None, True
        self._buf, self._buffered, self._queued, self._processed = [], 0, 0, 0

    def _alive(self):
        if not self._open:
            raise RuntimeError("pipeline already finished")

    def _flush(self):
        if not self._buffered:
            return
        if self._map is None:
            self._map = _run(_api.default_context().voxel_map, self._voxel_size)
        chunk = np.concatenate(self._buf) if len(self._buf) > 1 else self._buf[0]
        self._buf, n, self._buffered = [], self._buffered, 0
        _run(self._map.insert, chunk)
        self._processed += n

    def _push(self, pts):
        self._buf.append(pts)
        self._buffered += len(pts)
        self._queued += len(pts)
        if self._buffered >= self._BATCH:
            self._flush()

    def send(self, arr):
        self._alive()
        self._push(_point3(arr))

    def send_batch(self, arr):
        self._alive()
        pts = _nx3(arr)
        if len(pts):
            self._push(pts)
        return len(pts)

    def try_send(self, arr):
        """always True: there is no bounded queue here, so nothing is dropped"""
        self.send(arr)
        return True

    def metrics(self):
        self._alive()
        return RealtimeMetrics(self._queued, self._processed, 0)

    def finish(self):
        self._alive()
        self._open = False
        try:
            self._flush()
            if self._map is None:
                return PointCloud()
            return PointCloud(np.ascontiguousarray(_run(self._map.extract), np.float32))
        finally:
            if self._map is not None:
                self._map.close()
                self._map = None


class ShotVariant:
    """ShotVariant (features.rs:316-323)"""
    Standard, UniqueShapeContext = "shot", "usc"


class ShotConfig:
    """ShotConfig (features.rs:326-344): the reference's field names and defaults"""

    def __init__(self, search_radius=0.2, k_neighbors=10, variant=ShotVariant.Standard):
        self.search_radius, self.k_neighbors, self.variant = search_radius, k_neighbors, variant

    def __repr__(self):
        return f"ShotConfig(search_radius={self.search_radius}, k_neighbors={self.k_neighbors}, variant={self.variant!r})"


def extract_shot_features_with_normals(cloud, config=None):
    """extract_shot_features_with_normals (features.rs:605-645) over include/threecrate_hip_shot.h, which lists the deviations (an f64 frame,
    a canonical sign at an even vote): a NormalPointCloud -> one list of 352 (SHOT) or 128 (USC) floats per point"""
    config = ShotConfig() if config is None else config
    if len(cloud) == 0:
        return []
    d = _run(lambda: _api.default_context().extract_shot_features(cloud._pn, config.search_radius, config.k_neighbors, config.variant))
    return d.tolist()


class PoissonConfig:
    """PoissonConfig (poisson.rs:8-43) where its names have a meaning on a dense grid: depth (default 6, what the reference's clamp makes
    of its default 8) and scale; point_weight, max_iterations, tolerance and min_density are this library's (include/threecrate_hip_poisson.h)"""

    def __init__(self, depth=6, scale=1.1, point_weight=0.0, max_iterations=200, tolerance=1e-5, min_density=0.0):
        self.depth, self.scale, self.point_weight = depth, scale, point_weight
        self.max_iterations, self.tolerance, self.min_density = max_iterations, tolerance, min_density

    def __repr__(self):
        return (f"PoissonConfig(depth={self.depth}, scale={self.scale}, point_weight={self.point_weight}, max_iterations={self.max_iterations}, "
                f"tolerance={self.tolerance}, min_density={self.min_density})")


def poisson_reconstruct(cloud, config=None):
    """poisson_reconstruct (the wheel's name; poisson_reconstruction, poisson.rs:53-150) over include/threecrate_hip_poisson.h, which keeps
    the reference's entry checks and replaces its octree solver with a dense-grid solve: a NormalPointCloud -> a closed TriangleMesh"""
    if len(cloud) == 0:                                     # poisson.rs:57-59
        raise RuntimeError("Point cloud is empty")
    pn = cloud._pn
    v, f = _run(_api.default_context().poisson_reconstruct, np.ascontiguousarray(pn[:, 0:3]), np.ascontiguousarray(pn[:, 3:6]),
                PoissonConfig() if config is None else config)
    mesh = TriangleMesh()
    mesh._v, mesh._f = v, f
    return mesh


def poisson_reconstruct_with_normals(cloud, k=10, config=None):
    """poisson_reconstruction_with_normals (poisson.rs:167-180): estimate_normals(cloud, k), then poisson_reconstruct"""
    return poisson_reconstruct(estimate_normals(cloud, k), config)
