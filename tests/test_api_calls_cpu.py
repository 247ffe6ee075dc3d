"""The Python binding, call by call, without a GPU.

Every public method and function of threecrate_amd.api and threecrate_amd.distributed that reaches the library is driven
through a recording stand-in for libthreecrate_hip.so: an object whose every attribute is a function that appends
(name, normalised arguments) to a list and returns TC_OK.  GpuContext._order / _release land in the same list.  What is
recorded per scenario -- the sequence of library calls with their argument values, the ordering calls, and the shape of
what came back (or the exception) -- is compared with tests/golden/api_calls.json, which

    python tests/test_api_calls_cpu.py --record

wrote on the commit BEFORE the binding was rewritten around the array adapters (dbb2449).  The fixture also holds the
argtypes / restype of every export as _lib.load() set them on that commit.

Normalisation: integers and floats as they are; a byref struct field by field; a pointer as the array it points into
(an input the scenario handed in: its label and the byte offset, which is 0 or 12 for the normals pointer; a buffer the
call allocated: empty or zeros, dtype, shape, device); the 7-float start pose by value.  np.empty / torch.empty are
wrapped while a scenario runs: they fill the buffer with 0xFF bytes (every correspondence reads "none", so results are
deterministic) and allocate "cuda" requests on the CPU, which is what lets torch CPU tensors stand in for device ones.
"""
import contextlib
import ctypes as C
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from threecrate_amd import _lib, api, distributed as D  # noqa: E402

FIXTURE = os.path.join(ROOT, "tests", "golden", "api_calls.json")

_rng = np.random.default_rng(0)
DATA = {
    "P": _rng.random((10, 3), dtype=np.float32), "Q": _rng.random((10, 3), dtype=np.float32),
    "N3": _rng.random((10, 3), dtype=np.float32), "N6": _rng.random((10, 6), dtype=np.float32),
    "NFLAT": _rng.random(30, dtype=np.float32), "N3SHORT": _rng.random((9, 3), dtype=np.float32),
    "PN": _rng.random((10, 6), dtype=np.float32), "ONE": _rng.random(3, dtype=np.float32),
    "E": np.zeros((0, 3), np.float32), "K4": _rng.random((10, 4), dtype=np.float32),
    "INIT": np.array([0, 0, 0.1, 0.99, 0.1, 0.2, 0.3], np.float32),
}


def _base(x):
    if isinstance(x, np.ndarray):
        return x.ctypes.data, x.nbytes
    return x.data_ptr(), x.numel() * x.element_size()


class FakeLib:
    """every attribute is a function: record, hand out a handle for every `T **out`, return TC_OK (the two size getters: 10, the
    size of every cloud here)"""

    def __init__(self, harness):
        self._harness = harness

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        h = self._harness

        def fn(*args):
            h.calls.append([name, [h.norm(a) for a in args]])
            for a in args:
                if type(a).__name__ == "CArgObject" and isinstance(a._obj, C.c_void_p):
                    a._obj.value = h.next_handle
                    h.next_handle += 1
            return 10 if name in ("tc_cloud_size", "tc_search_index_size") else _lib.TC_OK
        return fn


class Harness:
    def __init__(self, kind):
        self.kind, self.calls, self.inputs, self.allocs, self.next_handle = kind, [], [], [], 0x2000
        self.lib = FakeLib(self)
        ctx = api.GpuContext.__new__(api.GpuContext)
        ctx._L, ctx._h, ctx.device, ctx.stream = self.lib, C.c_void_p(0x1000), 0, None
        ctx._order = lambda dev: self.calls.append(["_order", str(dev)])
        ctx._release = lambda dev: self.calls.append(["_release", str(dev)])
        self.ctx = ctx
        self.inputs.append(("IDENTITY", api.IDENTITY))

    def a(self, label, kind=None):
        """a fresh copy of DATA[label] in this scenario's input kind (float32, contiguous: the binding takes it in place)"""
        arr = DATA[label].copy()
        self.inputs.append((label, arr))
        return torch.from_numpy(arr) if (kind or self.kind) == "torch" else arr

    def comm(self):
        return D.Comm(self.ctx, C.c_void_p(0x3000), 0, 1)

    # ---- normalisation ----
    def pointer(self, p):
        for label, arr in self.inputs:
            b, nb = _base(arr)
            if b <= p < b + max(nb, 1):
                rec = {"in": label, "off": p - b}
                if nb <= 64 and isinstance(arr, np.ndarray):
                    rec["values"] = [float(v) for v in arr.reshape(-1)]
                return rec
        for kind, arr, dev in self.allocs:
            b, nb = _base(arr)
            if b and b <= p < b + max(nb, 1):
                return {"alloc": kind, "dtype": str(arr.dtype), "shape": list(arr.shape), "device": dev, "off": p - b}
        return "unknown-pointer"

    def norm(self, a):
        if a is None or isinstance(a, (bool, float, str)):
            return a
        if isinstance(a, int):
            return self.pointer(a) if a >= 1 << 32 else a
        if isinstance(a, bytes):
            return a.decode()
        if type(a).__name__ == "CArgObject":
            return {"ref": "new-handle" if isinstance(a._obj, C.c_void_p) else self.norm(a._obj)}
        if isinstance(a, C.c_void_p):
            return {"vp": a.value}
        if isinstance(a, C.Structure):
            out = {"struct": type(a).__name__}
            for name, typ in a._fields_:
                v = getattr(a, name)
                if isinstance(typ, type) and issubclass(typ, C._Pointer):
                    out[name] = [self.norm(v[i]) for i in range(a.n_levels)] if v else None
                else:
                    out[name] = self.norm(v)
            return out
        if isinstance(a, C.Array):
            if len(a) > 8:
                return {"array": type(a).__name__}
            return [self.norm(v) for v in a]
        if isinstance(a, C._SimpleCData):
            return {"c": type(a).__name__, "value": self.norm(a.value)}
        if isinstance(a, list):
            return [self.norm(v) for v in a]
        if callable(a):
            return "callback"
        raise TypeError(f"argument of type {type(a)}")

    def result(self, v):
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, np.ndarray):
            out = {"numpy": str(v.dtype), "shape": list(v.shape)}
            if v.size <= 16 and (v.dtype.kind in "iu" or np.isfinite(v).all()):
                out["values"] = [float(x) for x in v.reshape(-1)]
            return out
        if isinstance(v, torch.Tensor):
            return {"torch": str(v.dtype), "shape": list(v.shape), "device": str(v.device)}
        if isinstance(v, (tuple, list)):
            return [self.result(x) for x in v]
        if isinstance(v, dict):
            return {k: self.result(x) for k, x in v.items()}
        if dataclasses.is_dataclass(v):
            return {"type": type(v).__name__, **{f.name: self.result(getattr(v, f.name)) for f in dataclasses.fields(v)}}
        if isinstance(v, np.generic):
            return float(v)
        return {"object": type(v).__name__}


@contextlib.contextmanager
def patched_allocators(h):
    saved = (np.empty, np.zeros, torch.empty, torch.zeros, torch.empty_like)

    def host(kind, orig):
        def f(*a, **k):
            out = orig(*a, **k)
            if kind == "empty" and out.ndim:
                out.view(np.uint8).fill(0xFF)
            h.allocs.append((kind, out, "numpy"))
            return out
        return f

    def dev(kind, orig):
        def f(*a, **k):
            want = k.get("device")
            if want is not None and torch.device(want).type == "cuda":
                k["device"] = "cpu"
            out = orig(*a, **k)
            if kind == "empty" and out.numel():
                out.view(torch.uint8).fill_(0xFF)
            h.allocs.append((kind, out, str(want if want is not None else out.device)))
            return out
        return f
    np.empty, np.zeros = host("empty", saved[0]), host("zeros", saved[1])
    torch.empty, torch.zeros, torch.empty_like = dev("empty", saved[2]), dev("zeros", saved[3]), dev("empty", saved[4])
    try:
        yield
    finally:
        np.empty, np.zeros, torch.empty, torch.zeros, torch.empty_like = saved


# ---- the scenarios --------------------------------------------------------------------------------------------------
SCENARIOS = {}
BOTH, HOST, TORCH, MIXED = ("numpy", "torch"), ("numpy",), ("torch",), ("mixed",)


def scenario(name, kinds=BOTH):
    def deco(fn):
        for k in kinds:
            SCENARIOS[f"{name}[{k}]"] = (fn, k)
        return fn
    return deco


CFG = api.NormalEstimationConfig(k_neighbors=7, radius=0.25, consistent_orientation=False, viewpoint=(1.0, 2.0, 3.0))
MODES = {"pairs": True, "none": False, "device": "device"}
INITS = {"identity": None, "pose": "INIT"}

scenario("ctx_misc", HOST)(lambda h: [h.ctx.trim(), h.ctx.profile_enable(2), h.ctx.profile_reset(), h.ctx.debug_counter("index_builds"),
                                      h.ctx.search_stats(), h.ctx.profile_read(), h.ctx.profile_read(minmax=True)])
scenario("normals_with_config")(lambda h: h.ctx.estimate_normals_with_config(h.a("P"), CFG))
scenario("normals")(lambda h: h.ctx.estimate_normals(h.a("P"), 8))
scenario("normals_empty", HOST)(lambda h: h.ctx.estimate_normals(h.a("E"), 8))
scenario("normals_radius")(lambda h: h.ctx.estimate_normals_radius(h.a("P"), 0.5, True))
scenario("compute_normals")(lambda h: h.ctx.compute_normals(h.a("P"), 8))
scenario("normals_slice", TORCH)(lambda h: h.ctx.estimate_normals_slice(h.a("P"), CFG, 2, 7))
scenario("normals_unsort", TORCH)(lambda h: h.ctx.normals_unsort(h.a("PN")))
scenario("knn_batch", HOST)(lambda h: h.ctx.find_k_nearest_batch(h.a("P"), h.a("Q"), 4))
scenario("knn_batch_k0", HOST)(lambda h: h.ctx.find_k_nearest_batch(h.a("P"), h.a("Q"), 0))
scenario("knn_one", HOST)(lambda h: h.ctx.find_k_nearest(h.a("P"), h.a("ONE"), 4))
scenario("radius_batch", HOST)(lambda h: h.ctx.find_radius_neighbors_batch(h.a("P"), h.a("Q"), 0.5, 6))
scenario("radius_one", HOST)(lambda h: h.ctx.find_radius_neighbors(h.a("P"), h.a("ONE"), 0.5))
scenario("voxel")(lambda h: h.ctx.voxel_grid_filter(h.a("P"), 0.1))
scenario("voxel_empty", HOST)(lambda h: h.ctx.voxel_grid_filter(h.a("E"), 0.1))
scenario("cluster_labels")(lambda h: h.ctx.extract_euclidean_clusters_labels(h.a("P"), 0.3, 2, 100))
scenario("clusters")(lambda h: h.ctx.extract_euclidean_clusters(h.a("P"), 0.3, 0, 100))
scenario("clusters_empty", HOST)(lambda h: h.ctx.extract_euclidean_clusters(h.a("E"), 0.3, 1, 100))
scenario("clusters_negative_size")(lambda h: h.ctx.extract_euclidean_clusters(h.a("P"), 0.3, -1, 100))
scenario("fpfh_with_normals")(lambda h: h.ctx.extract_fpfh_features_with_normals(h.a("PN"), 0.2, 5))
scenario("fpfh")(lambda h: h.ctx.extract_fpfh_features(h.a("P"), 0.2, 5))
scenario("fpfh_negative_k")(lambda h: h.ctx.extract_fpfh_features(h.a("P"), 0.2, -1))
for _m, _want in MODES.items():
    for _i, _init in INITS.items():
        def _a(h, label):
            return None if label is None else h.a(label, "numpy")
        scenario(f"icp_detailed_{_m}_{_i}")(lambda h, w=_want, i=_init: h.ctx.icp_detailed(h.a("P"), h.a("Q"), _a(h, i), 5, 0.5, 1e-5, w))
        scenario(f"p2plane_{_m}_{_i}")(lambda h, w=_want, i=_init: h.ctx.icp_point_to_plane_detailed(
            h.a("P"), h.a("Q"), h.a("N3"), _a(h, i), 5, 0.5, 1e-5, w))
        scenario(f"gicp_{_m}_{_i}")(lambda h, w=_want, i=_init: h.ctx.gicp(h.a("P"), h.a("Q"), _a(h, i), api.GicpConfig(7, 0.5, 1e-5, 6), w))
        scenario(f"kiss_{_m}_{_i}")(lambda h, w=_want, i=_init: h.ctx.kiss_icp(h.a("P"), h.a("Q"), _a(h, i), api.KissIcpConfig(0.5, 50.0, 0.1, 7), w))
        scenario(f"cloud_p2plane_{_m}_{_i}")(lambda h, w=_want, i=_init: _cloud_pair(h, lambda s, t: s.icp_point_to_plane(t, _a(h, i), 5, 0.5, 1e-5, w)))
        scenario(f"cloud_detailed_{_m}_{_i}")(lambda h, w=_want, i=_init: _cloud_pair(h, lambda s, t: s.icp_detailed(t, _a(h, i), 5, None, 1e-5, w)))
        scenario(f"sharded_p2plane_{_m}_{_i}", TORCH)(lambda h, w=_want, i=_init: _with_comm(h, lambda c: D.sharded_icp_point_to_plane(
            h.ctx, h.a("P"), h.a("Q"), h.a("N6"), _a(h, i), 5, 0.5, 1e-5, comm=c, correspondences=w)))
        scenario(f"sharded_detailed_{_m}_{_i}", TORCH)(lambda h, w=_want, i=_init: _with_comm(h, lambda c: D.sharded_icp_detailed(
            h.ctx, h.a("P"), h.a("Q"), _a(h, i), 5, 0.5, 1e-5, comm=c, correspondences=w, shard="spatial")))
        scenario(f"sharded_cloud_{_m}_{_i}", TORCH)(lambda h, w=_want, i=_init: _with_comm(h, lambda c: _sharded_cloud(h, c, i, w)))


def _cloud_pair(h, body):
    s, t = api.Cloud(h.ctx, h.a("P")), api.Cloud(h.ctx, h.a("Q"))
    try:
        return body(s, t)
    finally:
        s.close(), t.close()


def _with_comm(h, body):
    c = h.comm()
    try:
        return body(c)
    finally:
        c._h = None         # borrowed by the call: whether the call destroyed it is in the record, this is not


def _sharded_cloud(h, comm, init, want, **kw):
    t = api.Cloud(h.ctx, h.a("Q"))
    try:
        return D.sharded_icp_against_cloud(h.ctx, h.a("P"), t, None if init is None else h.a(init, "numpy"), 5, 0.5, 1e-5, comm=comm,
                                           correspondences=want, **kw)
    finally:
        t.close()


scenario("icp_detailed_defaults")(lambda h: h.ctx.icp_detailed(h.a("P"), h.a("Q")))
scenario("icp_detailed_empty_source", HOST)(lambda h: h.ctx.icp_detailed(h.a("E"), h.a("Q")))
scenario("icp_detailed_negative_dist")(lambda h: h.ctx.icp_detailed(h.a("P"), h.a("Q"), None, 5, -0.5))
scenario("icp_detailed_negative_dist_empty", HOST)(lambda h: h.ctx.icp_detailed(h.a("E"), h.a("Q"), None, 5, -0.5))
scenario("icp_detailed_negative_dist_no_iters")(lambda h: h.ctx.icp_detailed(h.a("P"), h.a("Q"), None, 0, -0.5))
scenario("p2p")(lambda h: h.ctx.icp_point_to_point(h.a("P"), h.a("Q"), None, 5, 1e-4, 0.5))
scenario("p2p_bad_threshold")(lambda h: h.ctx.icp_point_to_point(h.a("P"), h.a("Q"), None, 5, 0.0, 0.5))
scenario("p2p_bad_threshold_negative_dist")(lambda h: h.ctx.icp_point_to_point(h.a("P"), h.a("Q"), None, 5, 0.0, -0.5))
scenario("icp")(lambda h: h.ctx.icp(h.a("P"), h.a("Q"), None, 5))
scenario("icp_pose")(lambda h: h.ctx.icp(h.a("P"), h.a("Q"), h.a("INIT", "numpy"), 5))
scenario("multiscale", HOST)(lambda h: h.ctx.multiscale_icp_point_to_point(h.a("P"), h.a("Q")))
scenario("multiscale_config", HOST)(lambda h: h.ctx.multiscale_icp_point_to_point(h.a("P"), h.a("Q"), h.a("INIT"), api.MultiScaleIcpConfig(
    [api.IcpScaleLevel(0.3, 4), api.IcpScaleLevel(0.1, 6, 0.2)], 3, None, 1e-4)))
scenario("p2plane_n6")(lambda h: h.ctx.icp_point_to_plane_detailed(h.a("P"), h.a("Q"), h.a("N6"), None, 5, None, 1e-5, "device"))
scenario("p2plane_flat")(lambda h: h.ctx.icp_point_to_plane_detailed(h.a("P"), h.a("Q"), h.a("NFLAT"), None, 5))
scenario("p2plane_negative_dist")(lambda h: h.ctx.icp_point_to_plane_detailed(h.a("P"), h.a("Q"), h.a("N6"), None, 5, -1.0))
scenario("p2plane_negative_dist_short_normals")(lambda h: h.ctx.icp_point_to_plane_detailed(h.a("P"), h.a("Q"), h.a("N3SHORT"), None, 5, -1.0))
scenario("p2plane_plain")(lambda h: h.ctx.icp_point_to_plane(h.a("P"), h.a("Q"), h.a("N3"), None, 5))


# one argument of the other kind: the source picks the road, and its companions are converted for THAT road (a host array on the
# torch road has no .detach(); a torch tensor on the numpy road goes through np.asarray, which refuses a device tensor)
for _name, _call in {
    "icp_detailed": lambda h, p, q, n: h.ctx.icp_detailed(p, q, None, 5, 0.5),
    "icp_detailed_negative_dist": lambda h, p, q, n: h.ctx.icp_detailed(p, q, None, 5, -0.5),
    "p2p": lambda h, p, q, n: h.ctx.icp_point_to_point(p, q, None, 5, 1e-4, 0.5),
    "gicp": lambda h, p, q, n: h.ctx.gicp(p, q),
    "kiss": lambda h, p, q, n: h.ctx.kiss_icp(p, q),
    "icp": lambda h, p, q, n: h.ctx.icp(p, q, None, 5),
    "p2plane": lambda h, p, q, n: h.ctx.icp_point_to_plane_detailed(p, q, n, None, 5, 0.5),
}.items():
    for _kinds in ("tnn", "ntn", "ttn", "nnt", "tnt", "ntt") if _name == "p2plane" else ("tnn", "ntn"):
        scenario(f"mixed_{_name}_{_kinds}", MIXED)(lambda h, c=_call, k=_kinds: c(h, *(
            h.a(label, {"t": "torch", "n": "numpy"}[x]) for label, x in zip(("P", "Q", "N6"), k))))


@scenario("free_functions")
def _free_functions(h):
    P, Q, N, PN = h.a("P"), h.a("Q"), h.a("N6"), h.a("PN")
    return [api.estimate_normals(P, 8), api.estimate_normals_with_config(P, CFG), api.estimate_normals_radius(P, 0.5, False),
            api.voxel_grid_filter(P, 0.1), api.gpu_voxel_grid_filter(h.ctx, P, 0.1), api.extract_euclidean_clusters(P, 0.3, 1, 100),
            api.gpu_extract_euclidean_clusters(h.ctx, P, 0.3, 1, 100), api.extract_fpfh_features_with_normals(PN),
            api.extract_fpfh_features(P), api.icp(P, Q), api.icp_detailed(P, Q, None, 5), api.icp_point_to_point(P, Q, None, 5),
            api.gicp(P, Q, None), api.kiss_icp(P, Q, None), api.icp_point_to_point_default(P, Q, None, 5),
            api.icp_point_to_plane(P, Q, N, None, 5), api.icp_point_to_plane_detailed(P, Q, N, None, 5),
            api.gpu_estimate_normals(h.ctx, P, 8), api.gpu_icp(h.ctx, P, Q, 5, 1e-5, 0.5),
            api.gpu_icp_point_to_plane(h.ctx, P, Q, N, 5, 1e-5, 0.5)]


@scenario("batch_icp", HOST)
def _batch(h):
    jobs = [api.BatchICPJob(h.a("P"), h.a("Q"), 5, 1e-5, 0.5), api.BatchICPJob(h.a("Q"), h.a("P"), 6, 1e-4, -1.0)]
    return api.gpu_batch_icp([h.ctx], jobs)


@scenario("cloud")
def _cloud(h):
    c = api.Cloud(h.ctx, h.a("P"))
    out = [len(c), c.estimate_normals(8), c.estimate_normals(config=CFG, out=False), c.normals()]
    c.close(), c.close()
    return out


@scenario("cloud_set_normals", TORCH)
def _cloud_set_normals(h):
    c = api.Cloud(h.ctx, h.a("P"))
    c.set_normals(h.a("N3")), c.set_normals(h.a("N6")), c.set_normals(h.a("NFLAT"))
    c.close()


scenario("cloud_negative_dist")(lambda h: _cloud_pair(h, lambda s, t: s.icp_point_to_plane(t, None, 5, -1.0)))


@scenario("frame_stream", HOST)
def _frame_stream(h):
    out = []
    for md in (None, 0.7, -2.0):
        fs = api.FrameStream(h.ctx, 100, 0.3, 8, 5, md, 1e-5, api.BackpressureConfig(2))
        fs.send(h.a("P")), out.append(fs.try_send(h.a("K4")))
        out.append(fs.finish())
    fs = api.FrameStream(h.ctx, 100)
    try:
        fs.send(h.a("NFLAT"))
    except api.InvalidData as e:
        out.append(str(e))
    del fs                              # an unfinished stream destroys its handle when it goes
    return out


@scenario("search_index")
def _search_index(h):
    ix = api.SearchIndex(h.ctx, h.a("P"), 12)
    out = [len(ix), ix.find_k_nearest_batch(h.a("Q"), 4), ix.find_radius_neighbors_batch(h.a("Q"), 0.5, 6),
           ix.find_radius_neighbors_batch(h.a("Q"), -1.0, 0)]
    ix.close(), ix.close()
    return out


@scenario("search_index_host_queries", HOST)
def _search_index_host(h):
    ix = api.SearchIndex(h.ctx, h.a("P"))
    out = [ix.radius_counts(h.a("Q"), 0.5), ix.find_radius_neighbors_all(h.a("Q"), 0.5), ix.find_k_nearest(h.a("ONE"), 4),
           ix.find_radius_neighbors(h.a("ONE"), 0.5), ix.find_k_nearest_batch(h.a("E"), 4)]
    ix.close()
    return out


scenario("read_kitti_bin", HOST)(lambda h: api.read_kitti_bin("/nonexistent/scan.bin"))


@scenario("comm", HOST)
def _comm(h):
    out = []
    for make in (D.Comm.local, D.Comm.rccl_single, D.Comm.from_group):
        c = make(h.ctx)
        out.append([c.rank, c.size])
        c.close(), c.close()
    return out


scenario("sharded_p2plane_own_comm", TORCH)(lambda h: D.sharded_icp_point_to_plane(h.ctx, h.a("P"), h.a("Q"), h.a("N3"), None, 5, correspondences=True))
scenario("sharded_p2plane_local_slice", TORCH)(lambda h: _with_comm(h, lambda c: D.sharded_icp_point_to_plane(
    h.ctx, h.a("P"), h.a("Q"), h.a("NFLAT"), None, 5, comm=c, source_is_local_slice=True)))
scenario("sharded_p2plane_index", TORCH)(lambda h: _with_comm(h, lambda c: D.sharded_icp_point_to_plane(
    h.ctx, h.a("P"), h.a("Q"), h.a("N3"), None, 5, comm=c, shard="index")))
scenario("sharded_p2plane_bad_shard", TORCH)(lambda h: D.sharded_icp_point_to_plane(h.ctx, h.a("P"), h.a("Q"), h.a("N3"), None, 5, shard="rows"))
scenario("sharded_p2plane_negative_dist", TORCH)(lambda h: D.sharded_icp_point_to_plane(h.ctx, h.a("P"), h.a("Q"), h.a("N3"), None, 5, -1.0))
scenario("sharded_p2plane_negative_dist_short_normals", TORCH)(lambda h: _with_comm(h, lambda c: D.sharded_icp_point_to_plane(
    h.ctx, h.a("P"), h.a("Q"), h.a("N3SHORT"), None, 5, -1.0, comm=c)))
scenario("sharded_detailed_own_comm", TORCH)(lambda h: D.sharded_icp_detailed(h.ctx, h.a("P"), h.a("Q"), None, 5))
scenario("sharded_detailed_negative_dist", TORCH)(lambda h: D.sharded_icp_detailed(h.ctx, h.a("P"), h.a("Q"), None, 0, -1.0))
scenario("sharded_cloud_own_comm", TORCH)(lambda h: _sharded_cloud(h, None, None, False, point_to_plane=False))
scenario("sharded_cloud_negative_dist", TORCH)(lambda h: _with_comm(h, lambda c: _sharded_cloud_negative(h, c)))


def _sharded_cloud_negative(h, comm):
    t = api.Cloud(h.ctx, h.a("Q"))
    try:
        return D.sharded_icp_against_cloud(h.ctx, h.a("P"), t, None, 5, -1.0, comm=comm, source_is_local_slice=True)
    finally:
        t.close()


scenario("sharded_normals", TORCH)(lambda h: _with_comm(h, lambda c: D.sharded_estimate_normals(h.ctx, h.a("P"), 8, comm=c)))
scenario("sharded_normals_own_comm", TORCH)(lambda h: D.sharded_estimate_normals(h.ctx, h.a("P"), config=CFG))
scenario("sharded_normals_local", TORCH)(lambda h: _with_comm(h, lambda c: D.sharded_estimate_normals_local(h.ctx, h.a("P"), 8, comm=c)))
scenario("sharded_normals_local_own_comm", TORCH)(lambda h: D.sharded_estimate_normals_local(h.ctx, h.a("P"), config=CFG))
scenario("stepwise_normals", TORCH)(lambda h: D.stepwise_sharded_estimate_normals(h.ctx, h.a("P"), 8))
scenario("stepwise_icp_empty", TORCH)(lambda h: D.stepwise_sharded_icp_point_to_plane(h.ctx, h.a("E"), h.a("Q"), h.a("N3")))


@scenario("shard_backend", TORCH)
def _shard_backend(h):
    out = []
    for normals, md in (("N3", 0.5), ("N6", None), ("NFLAT", None)):
        be = D.HipShardBackend(h.ctx, h.a("P"), h.a("Q"), h.a(normals), h.a("INIT", "numpy"), md, 1e-5)
        sums = be.reduce()
        be.same_stream = True           # apply() waits for torch's CUDA stream otherwise: not on a CPU
        be.apply(sums)
        out += [be.done(), be.finish(5)]
    for normals, md in (("N3SHORT", 0.5), ("N3", -1.0)):
        try:
            D.HipShardBackend(h.ctx, h.a("P"), h.a("Q"), h.a(normals), api.IDENTITY, md, 1e-5)
        except api.Error as e:
            out.append([type(e).__name__, str(e)])
    return out


def run(name):
    fn, kind = SCENARIOS[name]
    h = Harness(kind)
    saved = _lib._lib, api._default_ctx
    _lib._lib, api._default_ctx = h.lib, h.ctx
    try:
        with patched_allocators(h):
            try:
                out = {"return": h.result(fn(h))}
            except Exception as e:      # noqa: BLE001 -- which exception a bad call raises is part of the record
                out = {"raise": type(e).__name__, "message": str(e)}
        out["calls"] = list(h.calls)
    finally:
        _lib._lib, api._default_ctx = saved
        h.ctx._h = None
    return json.loads(json.dumps(out))


def signatures():
    L = _lib.load()
    out = {}
    for name in sorted(_lib.EXPORTS):
        fn = getattr(L, name)
        out[name] = {"argtypes": None if fn.argtypes is None else [t.__name__ for t in fn.argtypes],
                     "restype": "None" if fn.restype is None else fn.restype.__name__}
    return out


def _fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def pytest_generate_tests(metafunc):
    if "scenario_name" in metafunc.fixturenames:
        metafunc.parametrize("scenario_name", sorted(SCENARIOS))


def test_scenarios_are_the_recorded_ones():
    assert sorted(SCENARIOS) == sorted(_fixture()["scenarios"])


def test_calls_match_the_recorded_parent(scenario_name):
    want, got = _fixture()["scenarios"][scenario_name], run(scenario_name)
    assert got["calls"] == want["calls"]
    assert got == want


def test_every_export_keeps_its_argtypes_and_restype():
    want, got = _fixture()["signatures"], signatures()
    assert sorted(got) == sorted(want)
    for name in want:
        assert got[name] == want[name], name


def test_exports_keep_their_content():
    assert sorted(_lib.EXPORTS) == sorted(_fixture()["signatures"]) and len(set(_lib.EXPORTS)) == len(_lib.EXPORTS) == 90


# ---- the helpers themselves ------------------------------------------------------------------------------------------
def test_points_from_host_arrays():
    a = np.arange(12, dtype=np.float64).reshape(4, 3)
    for given in (a, a[:, ::-1], np.asfortranarray(a), a.reshape(-1), a.tolist()):
        p = api._points(given)
        assert (p.n, p.is_torch, p.device) == (4, False, None)
        assert p.a.dtype == np.float32 and p.a.flags.c_contiguous and p.a.shape == (4, 3)
        assert p.ptr == p.a.ctypes.data
        np.testing.assert_array_equal(p.a, np.asarray(given, np.float32).reshape(4, 3))
    for given in (np.zeros((0, 3)), np.zeros(0), []):
        p = api._points(given)
        assert p.n == 0 and p.a.shape == (0, 3) and p.a.dtype == np.float32
    p6 = api._points(np.arange(12.0), cols=6)
    assert p6.n == 2 and p6.a.shape == (2, 6)
    f = np.ones((4, 3), np.float32)
    assert api._points(f).ptr == f.ctypes.data              # taken in place, no copy


def test_points_from_torch_tensors():
    a = torch.arange(12, dtype=torch.float64).reshape(4, 3)
    for given in (a, a.flip(1), a.t().contiguous().t(), a.reshape(-1), a.clone().requires_grad_()):
        p = api._points(given)
        assert (p.n, p.is_torch, p.device) == (4, True, torch.device("cpu"))
        assert p.a.dtype == torch.float32 and p.a.is_contiguous() and tuple(p.a.shape) == (4, 3) and not p.a.requires_grad
        assert p.ptr == p.a.data_ptr()
        assert torch.equal(p.a, given.detach().to(torch.float32).reshape(4, 3))
    f = torch.ones((4, 3))
    assert api._points(f).ptr == f.data_ptr()
    assert api._points(torch.zeros((0, 3))).n == 0


def test_a_chosen_road_converts_for_that_road():
    """the companions of a call's first array (target, normals) follow ITS road: the other kind raises or is brought to the host,
    it never goes to the library as it is"""
    import pytest
    host, dev = np.ones((4, 3), np.float32), torch.ones((4, 3))
    p = api._points(dev, on_device=False)                       # np.asarray: fine for a CPU tensor, TypeError for a device one
    assert not p.is_torch and isinstance(p.a, np.ndarray) and p.n == 4
    assert isinstance(api._normals_arg(dev, on_device=False)[3], np.ndarray)
    assert api._points(dev, on_device=True).is_torch and not api._points(host, on_device=False).is_torch
    for call in (lambda: api._points(host, on_device=True), lambda: api._normals_arg(host, on_device=True)):
        with pytest.raises(AttributeError, match="detach"):
            call()


def test_normals_arg_takes_three_layouts():
    for conv in (lambda x: x, torch.from_numpy):
        n3, n6, flat = (conv(np.ones(s, np.float32)) for s in ((5, 3), (5, 6), (15,)))
        base = (lambda x: x.data_ptr()) if conv is torch.from_numpy else (lambda x: x.ctypes.data)
        for given, want in ((n3, (0, 5, 3)), (n6, (12, 5, 6)), (flat, (0, 5, 3))):
            ptr, count, stride, keep = api._normals_arg(given)
            assert (ptr - base(given), count, stride) == want
            assert base(keep) == base(given)
        ptr, count, stride, keep = api._normals_arg(conv(np.ones((5, 6), np.float64)))      # converted: `keep` owns the copy
        assert (ptr - base(keep), count, stride) == (12, 5, 6)
        assert str(keep.dtype).endswith("float32")


def test_init7():
    assert api._init7(None) is api.IDENTITY
    np.testing.assert_array_equal(api.IDENTITY, np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
    for given in ([0, 0, 0.5, 0.5, 1, 2, 3], np.array([[0, 0, 0.5, 0.5, 1, 2, 3]], np.float64), (0, 0, 0.5, 0.5, 1, 2, 3)):
        i7 = api._init7(given)
        assert i7.dtype == np.float32 and i7.shape == (7,) and i7.flags.c_contiguous
        np.testing.assert_array_equal(i7, np.array([0, 0, 0.5, 0.5, 1, 2, 3], np.float32))


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_api_calls_cpu.py --record   (on the commit whose behaviour is the reference)")
    scen = {name: run(name) for name in sorted(SCENARIOS)}
    for name, rec in scen.items():
        if "raise" in rec:
            print(f"{name}: {rec['raise']}: {rec['message']}")
    with open(FIXTURE, "w") as f:
        f.write('{"recorded_on": "dbb2449",\n "scenarios": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in scen.items()))
        f.write('\n },\n "signatures": {\n')
        f.write(",\n".join(f"  {json.dumps(k)}: {json.dumps(v)}" for k, v in signatures().items()))
        f.write("\n }\n}\n")
    print(f"{len(scen)} scenarios, {sum(len(v['calls']) for v in scen.values())} calls -> {FIXTURE}")
