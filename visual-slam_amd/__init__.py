"""visual_slam_amd -- Python plumbing over the C ABI of libvslam_hip.so (include/vslam_hip.h).

The product is the shared library (hand-written HIP for gfx950 + C++ host code); this module only
loads it with ctypes so that tests/ and bench.py can drive the C ABI.  There is NO fallback: if the
library is missing or no MI355X is visible, `load()` / `Context()` raise.

The directory is named `visual-slam_amd` (the layout the build contract asks for); it is imported
under the module name `visual_slam_amd` -- see `__graft_entry__.load_package()`.
"""
import ctypes as C
import os
from pathlib import Path

import numpy as np

_DIR = Path(__file__).resolve().parent
_SO = _DIR / "libvslam_hip.so"
_LIB = None

u8p = C.POINTER(C.c_uint8)
i32p = C.POINTER(C.c_int32)
u32p = C.POINTER(C.c_uint32)
u64p = C.POINTER(C.c_uint64)
i64p = C.POINTER(C.c_int64)
f32p = C.POINTER(C.c_float)
f64p = C.POINTER(C.c_double)

STAGES = ["response", "select", "describe", "match", "match_finalize", "ba_linearize", "ba_schur",
          "ba_solve", "bow_transform", "bow_score", "ba_finish", "ba_step"]

SPD_PATHS = ["none", "dense_panels", "band_panels", "band_fused", "band_two_ended", "bcr", "bcr_cyclic"]  # VSL_SPD_PATH_*

OK = 0
CAM_DS, CAM_PINHOLE, CAM_EUCM, CAM_KB4 = 0, 1, 2, 3  # VSL_CAM_*
ERR = {-1: "VSL_ERR_INVALID", -2: "VSL_ERR_HIP", -3: "VSL_ERR_NOMEM", -4: "VSL_ERR_CAPACITY",
       -5: "VSL_ERR_NO_DEVICE", -6: "VSL_ERR_IO", -7: "VSL_ERR_NUMERIC"}


class VslError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("%s (%d): %s" % (ERR.get(code, "VSL_ERR_?"), code, msg))
        self.code = code


class BaProblem(C.Structure):
    _fields_ = [("n_cams", C.c_int32), ("n_lms", C.c_int32), ("n_obs", C.c_int32),
                ("cam_model", C.c_int32 * 2), ("poses", f64p), ("cam_fixed", u8p),
                ("cam_intr", i32p), ("intr", f64p), ("points", f64p), ("obs_cam", i32p),
                ("obs_lm", i32p), ("obs_uv", f64p)]


class BaOptions(C.Structure):
    _fields_ = [("use_huber", C.c_int32), ("huber_parameter", C.c_double),
                ("max_num_iterations", C.c_int32), ("verbosity", C.c_int32)]


class BaSummary(C.Structure):
    _fields_ = [("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("iterations", C.c_int32), ("successful_steps", C.c_int32),
                ("termination", C.c_int32), ("linearize_ms", C.c_double),
                ("schur_ms", C.c_double), ("solve_ms", C.c_double), ("total_ms", C.c_double)]


class BaRig(C.Structure):
    _fields_ = [("n_bodies", C.c_int32), ("body_poses", f64p), ("body_fixed", u8p), ("cam_body", i32p), ("T_b_c", f64p)]


class BaPcgRecord(C.Structure):
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("pivot_fail", C.c_int32), ("segments", C.c_int32),
                ("landmark_runs", C.c_int32), ("n_free", C.c_int32), ("rr", C.c_double), ("bb", C.c_double),
                ("alpha", C.c_double), ("beta", C.c_double)]


class PgoProblem(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("n_edges", C.c_int32), ("poses", f64p), ("node_fixed", u8p),
                ("edge_a", i32p), ("edge_b", i32p), ("edge_meas", f64p)]


def library_path():
    return _SO


def load():
    """dlopen libvslam_hip.so (raises if it has not been built)."""
    global _LIB
    if _LIB is None:
        if not _SO.exists():
            raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(there is no CPU fallback)" % _SO)
        try:
            # PyTorch-ROCm ships its own HIP runtime; when both live in one process the runtime that is
            # loaded FIRST must be torch's, otherwise torch later reports "No HIP GPUs are available".
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(str(_SO))
        L.vsl_version.restype = C.c_char_p
        L.vsl_last_error.restype = C.c_char_p
        L.vsl_last_error.argtypes = [C.c_void_p]
        L.vsl_ctx_stream.restype = C.c_void_p
        L.vsl_ctx_stream.argtypes = [C.c_void_p]
        L.vsl_frames_images_dev.restype = C.c_void_p
        L.vsl_frames_images_dev.argtypes = [C.c_void_p]
        _LIB = L
    return _LIB


def device_count():
    return load().vsl_device_count()


def _img(img):
    img = np.ascontiguousarray(img, dtype=np.uint8)
    assert img.ndim == 2
    return img, img.ctypes.data_as(u8p), img.shape[1], img.shape[0], C.c_size_t(img.strides[0])


def _img_rows(img):
    """Like _img, but a uint8 view with contiguous rows (a region of a wider buffer) is passed as it is, with its pitch."""
    if isinstance(img, np.ndarray) and img.dtype == np.uint8 and img.ndim == 2 and img.strides[1] == 1 and \
            img.strides[0] >= img.shape[1]:
        return img, img.ctypes.data_as(u8p), img.shape[1], img.shape[0], C.c_size_t(img.strides[0])
    return _img(img)


def _mat9(M):
    return None if M is None else np.ascontiguousarray(np.asarray(M, np.float64).reshape(9))


def _vec3(v):
    return None if v is None else np.ascontiguousarray(np.asarray(v, np.float64).reshape(3))


def _cam(cam):
    """(VSL_CAM_* model, intrinsics) -> (model, 8 doubles fx fy cx cy p1..p4, zero-padded)."""
    model, intr = cam
    i8 = np.zeros(8, np.float64)
    intr = np.asarray(intr, np.float64).reshape(-1)
    i8[:len(intr)] = intr
    return int(model), i8


class Context:
    """vsl_ctx: one HIP stream + scratch.  `stream` = an existing hipStream_t handle (int) to borrow."""

    def __init__(self, device=0, stream=None):
        self.L = load()
        h = C.c_void_p()
        if stream is None:
            rc = self.L.vsl_ctx_create(int(device), C.byref(h))
        else:
            rc = self.L.vsl_ctx_create_on_stream(int(device), C.c_void_p(stream), C.byref(h))
        if rc != OK:
            raise VslError(rc, self.L.vsl_last_error(None).decode())
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.vsl_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != OK:
            raise VslError(rc, self.L.vsl_last_error(self.h).decode())

    def synchronize(self):
        self._ck(self.L.vsl_ctx_synchronize(self.h))

    def stream(self):
        return self.L.vsl_ctx_stream(self.h)

    def wait_event(self, ev):
        """Device-side ordering: later work on this context starts after the work `ev` marked has completed."""
        self._ck(self.L.vsl_ctx_wait_event(self.h, ev.h))

    def set_profiling(self, on):
        self._ck(self.L.vsl_ctx_set_profiling(self.h, int(on)))

    def last_ba_layout(self):
        """(doubles of S, band form, bandwidth) of the last general-path bundle adjustment set up on this context; band form
        0 = dense, 1 = band (cameras in reverse Cuthill-McKee order), 2 = cyclic band (cameras as they came, the band
        closes around the loop), 3 = matrix-free (iterative Schur: no S, 0 doubles)."""
        e, b, w = C.c_int64(), C.c_int(), C.c_int()
        self._ck(self.L.vsl_ctx_last_ba_layout(self.h, C.byref(e), C.byref(b), C.byref(w)))
        return e.value, b.value, w.value

    def reset_profiling(self):
        self._ck(self.L.vsl_ctx_reset_profiling(self.h))

    def stage_ms(self):
        out = {}
        for i, name in enumerate(STAGES):
            ms, n = C.c_double(), C.c_int64()
            self._ck(self.L.vsl_ctx_stage_ms(self.h, i, C.byref(ms), C.byref(n)))
            out[name] = (ms.value, n.value)
        return out

    def set_tie_eps(self, eps):
        self._ck(self.L.vsl_ctx_set_tie_eps(self.h, C.c_double(eps)))

    def sqrt_check(self, lo_bits, hi_bits):
        """Mismatches between the response kernel's square root and sqrtf over the float bit patterns [lo, hi]."""
        n = C.c_ulonglong(0)
        self._ck(self.L.vsl_diag_sqrt_check(self.h, C.c_uint32(int(lo_bits)), C.c_uint32(int(hi_bits)), C.byref(n)))
        return int(n.value)

    def set_diagnostic(self, name, value):
        self._ck(self.L.vsl_ctx_set_diagnostic(self.h, name.encode(), C.c_int(int(value))))

    def last_spd_path(self):
        """(path, block, n_blocks, levels) of the last SPD solve on this context: path is a name from SPD_PATHS; block,
        n_blocks and levels describe the block cyclic reduction and are 0 on the other paths."""
        p, B, nb, lv = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self._ck(self.L.vsl_ctx_last_spd_path(self.h, C.byref(p), C.byref(B), C.byref(nb), C.byref(lv)))
        return SPD_PATHS[p.value], B.value, nb.value, lv.value

    def spd_solve(self, S, b, half_bandwidth=-1):
        """Solves S x = b with the reduced-camera-system solver (dense, or band storage when half_bandwidth >= 0)."""
        S = np.ascontiguousarray(S, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        n = len(b)
        assert S.shape == (n, n)
        x = np.zeros(n, np.float64)
        self._ck(self.L.vsl_spd_solve(self.h, S.ctypes.data_as(f64p), b.ctypes.data_as(f64p), n, int(half_bandwidth),
                                      x.ctypes.data_as(f64p)))
        return x

    def spd_solve_cyclic(self, S, b, half_bandwidth):
        """Solves S x = b for a CYCLIC band matrix (non-zeros within cyclic distance half_bandwidth of the diagonal)."""
        S = np.ascontiguousarray(S, np.float64)
        b = np.ascontiguousarray(b, np.float64)
        n = len(b)
        assert S.shape == (n, n)
        x = np.zeros(n, np.float64)
        self._ck(self.L.vsl_spd_solve_cyclic(self.h, S.ctypes.data_as(f64p), b.ctypes.data_as(f64p), n, int(half_bandwidth),
                                             x.ctypes.data_as(f64p)))
        return x

    def spd_inverse_band(self, S, half_bandwidth=-1, cyclic=False):
        """The entries of S^-1 inside the (cyclic) band of S, everything else exactly 0 (vsl_spd_inverse_band: selected
        inversion on the band Cholesky factor); the full inverse when half_bandwidth < 0 or the band is the whole matrix."""
        S = np.ascontiguousarray(S, np.float64)
        n = S.shape[0] if S.ndim == 2 else 0
        assert S.size == n * n
        Z = np.zeros((n, n), np.float64)
        self._ck(self.L.vsl_spd_inverse_band(self.h, S.ctypes.data_as(f64p), n, int(half_bandwidth), int(bool(cyclic)),
                                             Z.ctypes.data_as(f64p)))
        return Z

    # ---- keypoints.h drop-ins (host buffers)
    def detect_describe(self, img, num_features=1500, rotate=True):
        img, p, w, h, pitch = _img(img)
        cap = num_features
        xy = np.zeros((cap, 2), np.float64)
        ang = np.zeros(cap, np.float64)
        desc = np.zeros((cap, 4), np.uint64)
        n = C.c_int32()
        self._ck(self.L.vsl_detect_describe(self.h, p, w, h, pitch, int(num_features), int(rotate), cap,
                                            xy.ctypes.data_as(f64p), ang.ctypes.data_as(f64p),
                                            desc.ctypes.data_as(u64p), C.byref(n)))
        return xy[:n.value].copy(), ang[:n.value].copy(), desc[:n.value].copy()

    def detect_keypoints(self, img, num_features=1500):
        img, p, w, h, pitch = _img(img)
        xy = np.zeros((num_features, 2), np.float64)
        n = C.c_int32()
        self._ck(self.L.vsl_detect_keypoints(self.h, p, w, h, pitch, int(num_features), num_features,
                                             xy.ctypes.data_as(f64p), C.byref(n)))
        return xy[:n.value].copy()

    def compute_angles(self, img, corners, rotate=True):
        img, p, w, h, pitch = _img(img)
        corners = np.ascontiguousarray(corners, np.float64).reshape(-1, 2)
        ang = np.zeros(len(corners), np.float64)
        self._ck(self.L.vsl_compute_angles(self.h, p, w, h, pitch, corners.ctypes.data_as(f64p),
                                           len(corners), int(rotate), ang.ctypes.data_as(f64p)))
        return ang

    def compute_descriptors(self, img, corners, angles):
        img, p, w, h, pitch = _img(img)
        corners = np.ascontiguousarray(corners, np.float64).reshape(-1, 2)
        angles = np.ascontiguousarray(angles, np.float64)
        desc = np.zeros((len(corners), 4), np.uint64)
        self._ck(self.L.vsl_compute_descriptors(self.h, p, w, h, pitch, corners.ctypes.data_as(f64p),
                                                angles.ctypes.data_as(f64p), len(corners),
                                                desc.ctypes.data_as(u64p)))
        return desc

    def min_eig_response(self, img):
        img, p, w, h, pitch = _img(img)
        out = np.zeros((h, w), np.float32)
        self._ck(self.L.vsl_min_eig_response(self.h, p, w, h, pitch, out.ctypes.data_as(f32p)))
        return out

    def match_descriptors(self, d1, d2, threshold=70, dist_2_best=1.2):
        d1 = np.ascontiguousarray(d1, np.uint64).reshape(-1, 4)
        d2 = np.ascontiguousarray(d2, np.uint64).reshape(-1, 4)
        pairs = np.zeros((max(1, min(len(d1), len(d2))), 2), np.int32)
        n = C.c_int32()
        self._ck(self.L.vsl_match_descriptors(self.h, d1.ctypes.data_as(u64p), len(d1),
                                              d2.ctypes.data_as(u64p), len(d2), int(threshold),
                                              C.c_double(dist_2_best), pairs.ctypes.data_as(i32p),
                                              C.byref(n)))
        return pairs[:n.value].copy()

    # ---- matching_utils.h drop-in
    def find_inliers_essential(self, cam_a, cam_b, E, kp_a_xy, kp_b_xy, matches, threshold=1e-3, R=None, t=None,
                               points=True):
        """vsl_find_inliers_essential: findInliersEssential on host buffers for one pair, plus (with R, t = R_0_1, t_0_1
        and points=True) the midpoint triangulation of every inlier.  Returns (pairs (n, 2) int32, points (n, 3) or None)."""
        E9, R9, t3 = _mat9(E), _mat9(R), _vec3(t)
        (ma, ia), (mb, ib) = _cam(cam_a), _cam(cam_b)
        a = np.ascontiguousarray(kp_a_xy, np.float64).reshape(-1, 2)
        b = np.ascontiguousarray(kp_b_xy, np.float64).reshape(-1, 2)
        m = np.ascontiguousarray(matches, np.int32).reshape(-1, 2)
        want = bool(points) and R9 is not None and t3 is not None
        out = np.zeros((max(len(m), 1), 2), np.int32)
        pts = np.zeros((max(len(m), 1), 3), np.float64)
        n = C.c_int32()
        self._ck(self.L.vsl_find_inliers_essential(
            self.h, ma, ia.ctypes.data_as(f64p), mb, ib.ctypes.data_as(f64p), E9.ctypes.data_as(f64p),
            a.ctypes.data_as(f64p), len(a), b.ctypes.data_as(f64p), len(b), m.ctypes.data_as(i32p), len(m),
            C.c_double(threshold), R9.ctypes.data_as(f64p) if R9 is not None else None,
            t3.ctypes.data_as(f64p) if t3 is not None else None, out.ctypes.data_as(i32p),
            pts.ctypes.data_as(f64p) if want else None, C.byref(n)))
        return out[:n.value].copy(), (pts[:n.value].copy() if want else None)

    # ---- vo_utils.h drop-ins
    def project_landmarks(self, pose7, model, intr8, width, height, points, cam_z_threshold=0.1):
        pose7 = np.ascontiguousarray(pose7, np.float64)
        intr8 = np.ascontiguousarray(intr8, np.float64)
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        n = len(points)
        uv = np.zeros((max(n, 1), 2), np.float64)
        idx = np.zeros(max(n, 1), np.int32)
        m = C.c_int32()
        self._ck(self.L.vsl_project_landmarks(self.h, pose7.ctypes.data_as(f64p), int(model), intr8.ctypes.data_as(f64p),
                                              int(width), int(height), points.ctypes.data_as(f64p), n,
                                              C.c_double(cam_z_threshold), uv.ctypes.data_as(f64p),
                                              idx.ctypes.data_as(i32p), C.byref(m)))
        return uv[:m.value].copy(), idx[:m.value].copy()

    def find_matches_landmarks(self, kp_xy, kp_desc, proj_uv, proj_lm, lm_obs_start, obs_desc, max_dist_2d=20.0,
                               threshold=70, dist_2_best=1.2):
        kp_xy = np.ascontiguousarray(kp_xy, np.float64).reshape(-1, 2)
        kp_desc = np.ascontiguousarray(kp_desc, np.uint64).reshape(-1, 4)
        proj_uv = np.ascontiguousarray(proj_uv, np.float64).reshape(-1, 2)
        proj_lm = np.ascontiguousarray(proj_lm, np.int32)
        lm_obs_start = np.ascontiguousarray(lm_obs_start, np.int32)
        obs_desc = np.ascontiguousarray(obs_desc, np.uint64).reshape(-1, 4)
        pairs = np.zeros((max(len(kp_xy), 1), 2), np.int32)
        m = C.c_int32()
        self._ck(self.L.vsl_find_matches_landmarks(self.h, kp_xy.ctypes.data_as(f64p), kp_desc.ctypes.data_as(u64p),
                                                   len(kp_xy), proj_uv.ctypes.data_as(f64p),
                                                   proj_lm.ctypes.data_as(i32p), len(proj_uv),
                                                   lm_obs_start.ctypes.data_as(i32p), len(lm_obs_start) - 1,
                                                   obs_desc.ctypes.data_as(u64p), C.c_double(max_dist_2d),
                                                   int(threshold), C.c_double(dist_2_best),
                                                   pairs.ctypes.data_as(i32p), C.byref(m)))
        return pairs[:m.value].copy()

    def fuse_search(self, poses, model, intr8, width, height, kp_xy, kp_desc, points, lm_obs_start, obs_desc,
                    cam_z_threshold=0.1, max_dist_2d=20.0, threshold=70, dist_2_best=1.2):
        """vsl_fuse_search: project_landmarks + find_matches_landmarks for every view in one call.  poses: (V, 7);
        kp_xy / kp_desc: one array per view.  Returns (list of per-view (n, 2) int32 pairs, n_projected[V])."""
        poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7)
        intr8 = np.ascontiguousarray(intr8, np.float64)
        V = len(poses)
        assert len(kp_xy) == V and len(kp_desc) == V
        xy = [np.asarray(a, np.float64).reshape(-1, 2) for a in kp_xy]
        ds = [np.asarray(a, np.uint64).reshape(-1, 4) for a in kp_desc]
        kp_start = np.concatenate([[0], np.cumsum([len(a) for a in xy])]).astype(np.int32)
        xy = np.ascontiguousarray(np.concatenate(xy + [np.zeros((0, 2))]), np.float64)
        ds = np.ascontiguousarray(np.concatenate(ds + [np.zeros((0, 4), np.uint64)]), np.uint64)
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        lm_obs_start = np.ascontiguousarray(lm_obs_start, np.int32)
        obs_desc = np.ascontiguousarray(obs_desc, np.uint64).reshape(-1, 4)
        pairs = np.zeros((max(len(xy), 1), 2), np.int32)
        pair_start = np.zeros(V + 1, np.int32)
        n_proj = np.zeros(max(V, 1), np.int32)
        self._ck(self.L.vsl_fuse_search(self.h, V, poses.ctypes.data_as(f64p), int(model), intr8.ctypes.data_as(f64p),
                                        int(width), int(height), kp_start.ctypes.data_as(i32p), xy.ctypes.data_as(f64p),
                                        ds.ctypes.data_as(u64p), len(points), points.ctypes.data_as(f64p),
                                        lm_obs_start.ctypes.data_as(i32p), obs_desc.ctypes.data_as(u64p),
                                        C.c_double(cam_z_threshold), C.c_double(max_dist_2d), int(threshold),
                                        C.c_double(dist_2_best), pairs.ctypes.data_as(i32p),
                                        pair_start.ctypes.data_as(i32p), n_proj.ctypes.data_as(i32p)))
        return [pairs[pair_start[v]:pair_start[v + 1]].copy() for v in range(V)], n_proj[:V].copy()

    def orb_detect_describe(self, img, num_features=1500):
        """ORB front end of compute_bow_vector: (kp[n, 5] = x, y, angle_deg, response, octave; desc[n, 32]).
        Every keypoint is returned: retainBest keeps all ties, so when the first buffer (2 * num_features + 512) is too
        small the call is repeated once with the total that vsl_orb_detect_describe reports."""
        img, p, w, h, pitch = _img_rows(img)
        cap = 2 * num_features + 512
        for _ in range(2):
            kp = np.zeros((max(cap, 1), 5), np.float32)
            desc = np.zeros((max(cap, 1), 32), np.uint8)
            n = C.c_int32()
            rc = self.L.vsl_orb_detect_describe(self.h, p, w, h, pitch, int(num_features), cap,
                                                kp.ctypes.data_as(C.POINTER(C.c_float)), desc.ctypes.data_as(u8p), C.byref(n))
            if rc != -4 or n.value <= cap:   # VSL_ERR_CAPACITY: n = the capacity that suffices
                break
            cap = n.value
        self._ck(rc)
        return kp[:n.value].copy(), desc[:n.value].copy()

    def orb_level_sizes(self, w, h):
        """(widths[8], heights[8]) of the ORB pyramid of a w x h image."""
        lw, lh = np.zeros(8, np.int32), np.zeros(8, np.int32)
        self._ck(self.L.vsl_orb_level_sizes(int(w), int(h), lw.ctypes.data_as(i32p), lh.ctypes.data_as(i32p)))
        return lw, lh

    def orb_stage_images(self, img, level):
        """Test / diagnostic: (pyramid level, FAST score image, NMS + border flags, blurred level) of one pyramid level,
        uint8 [H_level, W_level] each, after the same launches as orb_detect_describe."""
        img, p, w, h, pitch = _img_rows(img)
        lw, lh = self.orb_level_sizes(w, h)
        out = [np.zeros((lh[level], lw[level]), np.uint8) for _ in range(4)]
        self._ck(self.L.vsl_orb_stage_images(self.h, p, w, h, pitch, int(level), *[o.ctypes.data_as(u8p) for o in out]))
        return tuple(out)

    # ---- bundle adjustment
    def _ba_struct(self, arr):
        st = BaProblem()
        st.n_cams, st.n_lms, st.n_obs = len(arr.poses), len(arr.points), len(arr.obs_cam)
        st.cam_model[0], st.cam_model[1] = arr.cam_model
        st.poses = arr.poses.ctypes.data_as(f64p)
        st.cam_fixed = arr.cam_fixed.ctypes.data_as(u8p)
        st.cam_intr = arr.cam_intr.ctypes.data_as(i32p)
        st.intr = arr.intr.ctypes.data_as(f64p)
        st.points = arr.points.ctypes.data_as(f64p)
        st.obs_cam = arr.obs_cam.ctypes.data_as(i32p)
        st.obs_lm = arr.obs_lm.ctypes.data_as(i32p)
        st.obs_uv = arr.obs_uv.ctypes.data_as(f64p)
        return st

    @staticmethod
    def _ba_opts(use_huber, huber, max_iters, verbosity):
        o = BaOptions()
        o.use_huber, o.huber_parameter = int(use_huber), float(huber)
        o.max_num_iterations, o.verbosity = int(max_iters), int(verbosity)
        return o

    def bundle_adjust(self, arr, use_huber=True, huber=1.0, max_iters=20, verbosity=0):
        """arr: object with the numpy fields of include/vslam_hip.h's vsl_ba_problem (optimised in place)."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        s = BaSummary()
        self._ck(self.L.vsl_bundle_adjust(self.h, C.byref(st), C.byref(o), C.byref(s)))
        return s

    # ---- pose graph optimisation (loop_closure_utils.h:446-587)
    @staticmethod
    def _pgo_struct(arr):
        st = PgoProblem()
        st.n_nodes, st.n_edges = len(arr.poses), len(arr.edge_a)
        st.poses = arr.poses.ctypes.data_as(f64p)
        st.node_fixed = arr.node_fixed.ctypes.data_as(u8p)
        st.edge_a = arr.edge_a.ctypes.data_as(i32p)
        st.edge_b = arr.edge_b.ctypes.data_as(i32p)
        st.edge_meas = arr.edge_meas.ctypes.data_as(f64p)
        return st

    @staticmethod
    def _edge_info(arr, edge_info):
        """None, or the [E, 6, 6] float64 information matrices of arr's edges, contiguous.  Anything else is a ValueError
        here, before a native call sees it."""
        if edge_info is None:
            return None
        if not isinstance(edge_info, np.ndarray) or edge_info.dtype != np.float64 or edge_info.shape != (len(arr.edge_a), 6, 6):
            raise ValueError("edge_info: a float64 array of shape [%d, 6, 6] is needed" % len(arr.edge_a))
        return np.ascontiguousarray(edge_info)

    def _pgo_call(self, name, info, st, *args):
        """The unweighted symbol when info is None, else its _w form (edge_info sits directly after prob)."""
        if info is None:
            return self._ck(getattr(self.L, name)(self.h, C.byref(st), *args))
        return self._ck(getattr(self.L, name + "_w")(self.h, C.byref(st), info.ctypes.data_as(f64p), *args))

    def pose_graph_optimize(self, arr, use_huber=True, huber=1.0, max_iters=20, verbosity=0, *, edge_info=None):
        """arr: object with the numpy fields of vsl_pgo_problem (poses [N, 7] optimised in place).  edge_info: [E, 6, 6]
        float64 information matrices of the edges (vsl_pose_graph_optimize_w), None: identity."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        s = BaSummary()
        self._pgo_call("vsl_pose_graph_optimize", info, st, C.byref(o), C.byref(s))
        return s

    def pgo_linearize(self, arr, use_huber=True, huber=1.0, *, edge_info=None):
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.node_fixed == 0).sum())
        H, g = np.zeros((max(n, 1), max(n, 1))), np.zeros(max(n, 1))
        cost, nf = C.c_double(), C.c_int32()
        Hc = np.zeros(n * n)
        self._pgo_call("vsl_pgo_linearize", info, st, C.byref(o), Hc.ctypes.data_as(f64p), g.ctypes.data_as(f64p),
                       C.byref(cost), C.byref(nf))
        return Hc.reshape(n, n), g[:n].copy(), cost.value

    def pgo_linearize_stored(self, arr, use_huber=True, huber=1.0, jacobi_scale=False, *, edge_info=None):
        """The normal equations as the solver stores them for this graph, expanded to dense: H, g, cost and
        info = dict(storage = 0 dense / 1 band / 2 cyclic band, half_bandwidth, stray_nonzeros, n_free)."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.node_fixed == 0).sum())
        Hc, g = np.zeros(n * n), np.zeros(max(n, 1))
        cost, nf, storage, bw, stray = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        self._pgo_call("vsl_pgo_linearize_stored", info, st, C.byref(o), int(bool(jacobi_scale)), Hc.ctypes.data_as(f64p),
                       g.ctypes.data_as(f64p), C.byref(cost), C.byref(nf), C.byref(storage), C.byref(bw), C.byref(stray))
        return Hc.reshape(n, n), g[:n].copy(), cost.value, dict(storage=storage.value, half_bandwidth=bw.value,
                                                                 stray_nonzeros=stray.value, n_free=nf.value)

    def pgo_covariance(self, arr, nodes=None, use_huber=True, huber=1.0, *, edge_info=None):
        """Marginal covariances of the pose graph's nodes at arr's poses (vsl_pgo_covariance; nothing is optimised).
        nodes: node ids (None: all free nodes, ascending).  Returns (cov [n_q, 6, 6], storage) with storage = 0 dense /
        1 linear band / 2 folded ring: the route the call took.  edge_info as in pose_graph_optimize."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        nodes = np.flatnonzero(arr.node_fixed == 0) if nodes is None else nodes
        nodes = np.ascontiguousarray(nodes, np.int32).reshape(-1)
        cov = np.zeros((len(nodes), 6, 6))
        storage = C.c_int(-1)
        self._pgo_call("vsl_pgo_covariance", info, st, C.byref(o), nodes.ctypes.data_as(i32p), len(nodes),
                       cov.ctypes.data_as(f64p), C.byref(storage))
        return cov, storage.value

    def pgo_joint_covariance(self, arr, pairs, use_huber=True, huber=1.0, *, edge_info=None):
        """Joint marginal covariances of pairs of nodes (vsl_pgo_joint_covariance; nothing is optimised).  pairs: [n, 2]
        node ids (a, b); one of the two may be fixed (zero rows and columns).  Returns (cov [n, 12, 12] in the order
        (a, b), storage).  edge_info as in pose_graph_optimize."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        cov = np.zeros((len(a), 12, 12))
        storage = C.c_int(-1)
        self._pgo_call("vsl_pgo_joint_covariance", info, st, C.byref(o), a.ctypes.data_as(i32p), b.ctypes.data_as(i32p), len(a),
                       cov.ctypes.data_as(f64p), C.byref(storage))
        return cov, storage.value

    def pgo_edge_consistency(self, arr, cand_a, cand_b, cand_meas, meas_cov=None, use_huber=True, huber=1.0, *, edge_info=None):
        """Residual, residual covariance and chi-square of candidate edges (a, b, meas) against the graph as it stands
        (vsl_pgo_edge_consistency).  cand_meas: [n, 6]; meas_cov: [n, 6, 6] or None (zero).  Returns (resid [n, 6],
        resid_cov [n, 6, 6], chi2 [n], storage); chi2 is NaN where resid_cov + meas_cov is not positive definite.
        edge_info: information matrices of the GRAPH's edges (they shape the covariance, not the candidate's residual)."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        a = np.ascontiguousarray(cand_a, np.int32).reshape(-1)
        b = np.ascontiguousarray(cand_b, np.int32).reshape(-1)
        n = len(a)
        meas = np.ascontiguousarray(cand_meas, np.float64).reshape(n, 6)
        mc = None if meas_cov is None else np.ascontiguousarray(meas_cov, np.float64).reshape(n, 36)
        if len(b) != n:
            raise ValueError("cand_a and cand_b differ in length")
        resid, resid_cov, chi2 = np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros(n)
        storage = C.c_int(-1)
        self._pgo_call("vsl_pgo_edge_consistency", info, st, C.byref(o), a.ctypes.data_as(i32p), b.ctypes.data_as(i32p),
                       meas.ctypes.data_as(f64p), None if mc is None else mc.ctypes.data_as(f64p), n,
                       resid.ctypes.data_as(f64p), resid_cov.ctypes.data_as(f64p), chi2.ctypes.data_as(f64p), C.byref(storage))
        return resid, resid_cov, chi2, storage.value

    def pgo_far_solve(self, arr, b=None, max_near_distance=-1, use_huber=True, huber=1.0, *, edge_info=None):
        """Solves H x = b (b None: g) for the H, g of pgo_linearize by the band factor of the near edges plus the
        low-rank update of the far ones (vsl_pgo_far_solve).  max_near_distance >= 0 forces d*, -1 takes the plan's
        choice.  Returns (x, far_edges, half_bandwidth).  The switch of the solver itself is
        set_diagnostic("pgo_far_edges", 1); last_pgo_far() tells whether a solve took the route."""
        info = self._edge_info(arr, edge_info)
        st = self._pgo_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.node_fixed == 0).sum())
        if b is not None:
            b = np.ascontiguousarray(b, np.float64).reshape(-1)
            if len(b) != n:
                raise ValueError("b has %d entries, the problem %d unknowns" % (len(b), n))
        x = np.zeros(max(n, 1))
        k, bw = C.c_int(0), C.c_int(0)
        self._ck(self.L.vsl_pgo_far_solve(self.h, C.byref(st), None if info is None else info.ctypes.data_as(f64p), C.byref(o),
                                          None if b is None else b.ctypes.data_as(f64p), C.c_int(int(max_near_distance)),
                                          x.ctypes.data_as(f64p), C.byref(k), C.byref(bw)))
        return x[:n].copy(), k.value, bw.value

    def last_pgo_far(self):
        """dict(taken, far_edges, half_bandwidth, columns, solves) of the far-edge route in the last pose_graph_optimize
        on this context; zeros when it did not take the route."""
        t, k, bw, c, s = C.c_int(), C.c_int(), C.c_int(), C.c_int(), C.c_int64()
        self._ck(self.L.vsl_ctx_last_pgo_far(self.h, C.byref(t), C.byref(k), C.byref(bw), C.byref(c), C.byref(s)))
        return dict(taken=t.value, far_edges=k.value, half_bandwidth=bw.value, columns=c.value, solves=s.value)

    def bundle_adjust_intrinsics(self, arr, use_huber=True, huber=1.0, max_iters=20, verbosity=0):
        """optimize_intrinsics = true: optimises arr.poses / arr.points / arr.intr in place."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        out = BaSummary()
        self._ck(self.L.vsl_bundle_adjust_intrinsics(self.h, C.byref(st), C.byref(o), arr.intr.ctypes.data_as(f64p),
                                                     C.byref(out)))
        return out

    def ba_intrinsics_system(self, arr, inv_radius=0.0, use_huber=True, huber=1.0):
        """The first linearisation of bundle_adjust_intrinsics and one scaled, damped reduced system [poses | intrinsics]
        at 1 / radius = inv_radius, built and solved by the solve's own routines (vsl_ba_intrinsics_system): a dict with
        G [n_obs, 2, 8] (unscaled, no robustifier), scale [nt], S [nt, nt], rhs [nt], cost, d [nt], dl [n_lms, 3] (scaled
        variables), chol_ok, n_free; nt = 6 * n_free + 16.  Nothing in arr is changed."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        nf = int((arr.cam_fixed == 0).sum())
        nt = 6 * nf + 16
        G = np.zeros((len(arr.obs_cam), 2, 8))
        S, rhs, scale, d, dl = np.zeros((nt, nt)), np.zeros(nt), np.zeros(nt), np.zeros(nt), np.zeros((len(arr.points), 3))
        cost, ok = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_intrinsics_system(self.h, C.byref(st), C.byref(o), arr.intr.ctypes.data_as(f64p),
                                                 C.c_double(inv_radius), G.ctypes.data_as(f64p), scale.ctypes.data_as(f64p),
                                                 S.ctypes.data_as(f64p), rhs.ctypes.data_as(f64p), C.byref(cost),
                                                 d.ctypes.data_as(f64p), dl.ctypes.data_as(f64p), C.byref(ok)))
        return dict(G=G, scale=scale, S=S, rhs=rhs, cost=cost.value, d=d, dl=dl, chol_ok=ok.value, n_free=nf)

    def ba_linearize(self, arr, use_huber=True, huber=1.0, lm_first=0, lm_count=-1):
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.cam_fixed == 0).sum())
        S = np.zeros((n, n))
        g = np.zeros(n)
        cost, nf = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_linearize(self.h, C.byref(st), C.byref(o), int(lm_first), int(lm_count),
                                         S.ctypes.data_as(f64p), g.ctypes.data_as(f64p), C.byref(cost),
                                         C.byref(nf)))
        return S, g, cost.value

    def ba_fused_system(self, arr, inv_radius=0.0, use_huber=True, huber=1.0):
        """The scaled, damped reduced system of the fused iteration's first step (vsl_ba_fused_system): a dict with S
        [n, n] (full, as the device wrote it), rhs, scale_c, dc [n], cost, chol_ok, n_free -- or None when the fused
        kernels do not take the problem."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.cam_fixed == 0).sum())
        S, rhs, scale_c, dc = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
        cost, ok, nf, handled = C.c_double(), C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self.L.vsl_ba_fused_system(self.h, C.byref(st), C.byref(o), C.c_double(inv_radius), S.ctypes.data_as(f64p),
                                            rhs.ctypes.data_as(f64p), scale_c.ctypes.data_as(f64p), dc.ctypes.data_as(f64p),
                                            C.byref(cost), C.byref(ok), C.byref(nf), C.byref(handled)))
        if not handled.value:
            return None
        return dict(S=S, rhs=rhs, scale_c=scale_c, dc=dc, cost=cost.value, chol_ok=ok.value, n_free=nf.value)

    # ---- rig-constrained bundle adjustment: one pose per stereo frame (vsl_ba_rig, include/vslam_hip.h)
    def _ba_rig_structs(self, arr, rig):
        """The problem struct without cam_fixed (the rig calls ignore it) and the rig struct."""
        st = self._ba_struct(arr)
        rg = BaRig()
        rg.n_bodies = len(rig.body_poses)
        rg.body_poses = rig.body_poses.ctypes.data_as(f64p)
        rg.body_fixed = rig.body_fixed.ctypes.data_as(u8p)
        rg.cam_body = rig.cam_body.ctypes.data_as(i32p)
        rg.T_b_c = rig.T_b_c.ctypes.data_as(f64p)
        return st, rg

    def bundle_adjust_rig(self, arr, rig, use_huber=True, huber=1.0, max_iters=20, verbosity=0):
        """vsl_bundle_adjust_rig: optimises rig.body_poses and arr.points in place; arr.poses receives the camera poses
        derived from the final bodies.  rig: a RigArrays."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        s = BaSummary()
        self._ck(self.L.vsl_bundle_adjust_rig(self.h, C.byref(st), C.byref(rg), C.byref(o), C.byref(s)))
        return s

    def ba_rig_linearize(self, arr, rig, use_huber=True, huber=1.0):
        """(S, g, cost) of the reduced BODY system: Huber corrector, no scaling, no damping (vsl_ba_rig_linearize)."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * rig.n_free
        S, g = np.zeros((n, n)), np.zeros(n)
        cost, nf = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_rig_linearize(self.h, C.byref(st), C.byref(rg), C.byref(o), S.ctypes.data_as(f64p),
                                             g.ctypes.data_as(f64p), C.byref(cost), C.byref(nf)))
        assert nf.value == rig.n_free
        return S, g, cost.value

    def ba_rig_system(self, arr, rig, inv_radius=0.0, use_huber=True, huber=1.0):
        """The scaled, damped reduced body system of the rig solve's first step (vsl_ba_rig_system): a dict with S [n, n],
        rhs, scale_b, db [n], cost, chol_ok."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * rig.n_free
        S, rhs, scale_b, db = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
        cost, ok = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_rig_system(self.h, C.byref(st), C.byref(rg), C.byref(o), C.c_double(inv_radius),
                                          S.ctypes.data_as(f64p), rhs.ctypes.data_as(f64p), scale_b.ctypes.data_as(f64p),
                                          db.ctypes.data_as(f64p), C.byref(cost), C.byref(ok)))
        return dict(S=S, rhs=rhs, scale_b=scale_b, db=db, cost=cost.value, chol_ok=ok.value)

    # ---- rig bundle adjustment with the extrinsics as unknowns (include/vslam_hip.h)
    @staticmethod
    def _ext_args(T_b_c, ext_free):
        """(the caller's T_b_c as a contiguous float64 [2, 7] -- the SAME memory when it already is one --, the uint8 pair)."""
        T = np.asarray(T_b_c)
        if T.dtype != np.float64 or not T.flags.c_contiguous or T.size != 14:
            raise ValueError("T_b_c: a C-contiguous float64 array of 14 values (it is updated in place)")
        ef = np.ascontiguousarray([1 if f else 0 for f in ext_free], np.uint8)
        if ef.shape != (2,):
            raise ValueError("ext_free: two flags")
        return T, ef

    def bundle_adjust_rig_ext(self, arr, rig, T_b_c, ext_free=(0, 1), use_huber=True, huber=1.0, max_iters=20, verbosity=0):
        """vsl_bundle_adjust_rig_ext: bundle_adjust_rig with the extrinsic blocks flagged in ext_free estimated beside the
        bodies.  Updates rig.body_poses, arr.points, arr.poses and T_b_c ([2, 7] float64) in place; rig.T_b_c is ignored."""
        st, rg = self._ba_rig_structs(arr, rig)
        T, ef = self._ext_args(T_b_c, ext_free)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        s = BaSummary()
        self._ck(self.L.vsl_bundle_adjust_rig_ext(self.h, C.byref(st), C.byref(rg), ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p),
                                                  C.byref(o), C.byref(s)))
        return s

    def ba_rig_ext_linearize(self, arr, rig, T_b_c, ext_free=(0, 1), use_huber=True, huber=1.0):
        """(S, g, cost) of the reduced system over [free bodies | free extrinsic blocks]: Huber corrector, no scaling, no
        damping (vsl_ba_rig_ext_linearize)."""
        st, rg = self._ba_rig_structs(arr, rig)
        T, ef = self._ext_args(T_b_c, ext_free)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * (rig.n_free + int(ef.sum()))
        S, g = np.zeros((n, n)), np.zeros(n)
        cost, nb, ne = C.c_double(), C.c_int32(), C.c_int32()
        self._ck(self.L.vsl_ba_rig_ext_linearize(self.h, C.byref(st), C.byref(rg), ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p),
                                                 C.byref(o), S.ctypes.data_as(f64p), g.ctypes.data_as(f64p), C.byref(cost),
                                                 C.byref(nb), C.byref(ne)))
        assert nb.value == rig.n_free and ne.value == int(ef.sum())
        return S, g, cost.value

    def ba_rig_ext_system(self, arr, rig, T_b_c, inv_radius=0.0, ext_free=(0, 1), use_huber=True, huber=1.0):
        """The scaled, damped reduced system of the extrinsics solve's first step (vsl_ba_rig_ext_system): a dict with
        S [nt, nt], rhs, scale, d [nt], cost, chol_ok; nt = 6 * (free bodies + free blocks)."""
        st, rg = self._ba_rig_structs(arr, rig)
        T, ef = self._ext_args(T_b_c, ext_free)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * (rig.n_free + int(ef.sum()))
        S, rhs, scale, d = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
        cost, ok = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_rig_ext_system(self.h, C.byref(st), C.byref(rg), ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p),
                                              C.byref(o), C.c_double(inv_radius), S.ctypes.data_as(f64p), rhs.ctypes.data_as(f64p),
                                              scale.ctypes.data_as(f64p), d.ctypes.data_as(f64p), C.byref(cost), C.byref(ok)))
        return dict(S=S, rhs=rhs, scale=scale, d=d, cost=cost.value, chol_ok=ok.value)

    def global_bundle_adjust_rig(self, arr, rig, use_huber=True, huber=1.0, max_iters=20, verbosity=0):
        """vsl_global_bundle_adjust_rig: bundle_adjust_rig for a whole map -- the reduced body system gathered over the
        co-visible body pairs only and stored dense / band / cyclic band (last_ba_layout tells which)."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, max_iters, verbosity)
        s = BaSummary()
        self._ck(self.L.vsl_global_bundle_adjust_rig(self.h, C.byref(st), C.byref(rg), C.byref(o), C.byref(s)))
        return s

    def ba_rig_map_system(self, arr, rig, inv_radius=0.0, use_huber=True, huber=1.0):
        """ba_rig_system through the map route (vsl_ba_rig_map_system): S is the layout's storage expanded to dense [n, n]
        in ascending-body order; rhs, scale_b, db [n] in that order, cost, chol_ok."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * rig.n_free
        S, rhs, scale_b, db = np.zeros((n, n)), np.zeros(n), np.zeros(n), np.zeros(n)
        cost, ok = C.c_double(), C.c_int32()
        self._ck(self.L.vsl_ba_rig_map_system(self.h, C.byref(st), C.byref(rg), C.byref(o), C.c_double(inv_radius),
                                              S.ctypes.data_as(f64p), rhs.ctypes.data_as(f64p), scale_b.ctypes.data_as(f64p),
                                              db.ctypes.data_as(f64p), C.byref(cost), C.byref(ok)))
        return dict(S=S, rhs=rhs, scale_b=scale_b, db=db, cost=cost.value, chol_ok=ok.value)

    def ba_rig_covariance(self, arr, rig, bodies=None, cams=None, lms=None, use_huber=True, huber=1.0):
        """Marginal covariances of the RIG problem at rig's bodies / arr's points (vsl_ba_rig_covariance; nothing is
        optimised).  bodies: body ids (None: all free bodies), cams: camera ids (None: none), lms: landmark ids (None:
        none).  Returns (cov_body [n, 6, 6], cov_cam [m, 6, 6], cov_point [k, 3, 3], n_degenerate); a landmark whose own
        block is singular comes back as NaN and is counted."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, 0, 0)
        bodies = np.flatnonzero(rig.body_fixed == 0) if bodies is None else bodies
        bodies = np.ascontiguousarray(bodies, np.int32).reshape(-1)
        cams = np.ascontiguousarray([] if cams is None else cams, np.int32).reshape(-1)
        lms = np.ascontiguousarray([] if lms is None else lms, np.int32).reshape(-1)
        cb, cc, cl = np.zeros((len(bodies), 6, 6)), np.zeros((len(cams), 6, 6)), np.zeros((len(lms), 3, 3))
        nd = C.c_int(0)
        self._ck(self.L.vsl_ba_rig_covariance(self.h, C.byref(st), C.byref(rg), C.byref(o), bodies.ctypes.data_as(i32p),
                                              len(bodies), cb.ctypes.data_as(f64p), cams.ctypes.data_as(i32p), len(cams),
                                              cc.ctypes.data_as(f64p), lms.ctypes.data_as(i32p), len(lms),
                                              cl.ctypes.data_as(f64p), C.byref(nd)))
        return cb, cc, cl, nd.value

    def ba_rig_ext_covariance(self, arr, rig, T_b_c, ext_free=(0, 1), bodies=None, cams=None, lms=None, use_huber=True, huber=1.0):
        """Marginal covariances of the problem bundle_adjust_rig_ext adjusts, at rig's bodies, T_b_c and arr's points
        (vsl_ba_rig_ext_covariance; nothing is optimised, rig.T_b_c is ignored).  bodies: body ids (None: all free bodies),
        cams: camera ids (None: none), lms: landmark ids (None: none).  Returns a dict: cov_body [n, 6, 6], cov_ext
        [6 m, 6 m] over the m free blocks in ascending k, cov_body_ext [n, m, 6, 6], cov_cam [c, 6, 6], cov_point [k, 3, 3],
        n_degenerate.  VslError -7 (VSL_ERR_NUMERIC) when the window does not determine the extrinsic (a free gauge)."""
        st, rg = self._ba_rig_structs(arr, rig)
        T, ef = self._ext_args(T_b_c, ext_free)
        o = self._ba_opts(use_huber, huber, 0, 0)
        m = int(ef.sum())
        bodies = np.flatnonzero(rig.body_fixed == 0) if bodies is None else bodies
        bodies = np.ascontiguousarray(bodies, np.int32).reshape(-1)
        cams = np.ascontiguousarray([] if cams is None else cams, np.int32).reshape(-1)
        lms = np.ascontiguousarray([] if lms is None else lms, np.int32).reshape(-1)
        cb, cc, cl = np.zeros((len(bodies), 6, 6)), np.zeros((len(cams), 6, 6)), np.zeros((len(lms), 3, 3))
        ce, cx = np.zeros((6 * m, 6 * m)), np.zeros((len(bodies), m, 6, 6))
        nd = C.c_int(0)
        self._ck(self.L.vsl_ba_rig_ext_covariance(self.h, C.byref(st), C.byref(rg), ef.ctypes.data_as(u8p), T.ctypes.data_as(f64p),
                                                  C.byref(o), bodies.ctypes.data_as(i32p), len(bodies), cb.ctypes.data_as(f64p),
                                                  cams.ctypes.data_as(i32p), len(cams), cc.ctypes.data_as(f64p),
                                                  lms.ctypes.data_as(i32p), len(lms), cl.ctypes.data_as(f64p),
                                                  ce.ctypes.data_as(f64p) if m else None, cx.ctypes.data_as(f64p) if m else None,
                                                  C.byref(nd)))
        return dict(cov_body=cb, cov_ext=ce, cov_body_ext=cx, cov_cam=cc, cov_point=cl, n_degenerate=nd.value)

    def ba_rig_relative_pose_covariance(self, arr, rig, pairs, use_huber=True, huber=1.0):
        """ba_relative_pose_covariance for pairs of BODIES of the rig problem (vsl_ba_rig_relative_pose_covariance).
        pairs: [n, 2] body ids (a, b); one of the two may be fixed.  Returns (joint [n, 12, 12], meas [n, 6], cov
        [n, 6, 6], info [n, 6, 6], n_singular)."""
        st, rg = self._ba_rig_structs(arr, rig)
        o = self._ba_opts(use_huber, huber, 0, 0)
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        n = len(a)
        joint, meas, cov, info = np.zeros((n, 12, 12)), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
        ns = C.c_int(0)
        self._ck(self.L.vsl_ba_rig_relative_pose_covariance(self.h, C.byref(st), C.byref(rg), C.byref(o), a.ctypes.data_as(i32p),
                                                            b.ctypes.data_as(i32p), n, joint.ctypes.data_as(f64p),
                                                            meas.ctypes.data_as(f64p), cov.ctypes.data_as(f64p),
                                                            info.ctypes.data_as(f64p), C.byref(ns)))
        return joint, meas, cov, info, ns.value

    def ba_schur_apply(self, arr, x, use_huber=True, huber=1.0):
        """y = S x with the reduced camera system S of ba_linearize, never formed (vsl_ba_schur_apply)."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        nf = int((arr.cam_fixed == 0).sum())
        x = np.ascontiguousarray(x, np.float64).reshape(-1)
        if len(x) != 6 * nf:
            raise ValueError("x has %d entries, the problem %d unknowns" % (len(x), 6 * nf))
        y = np.zeros(6 * nf)
        self._ck(self.L.vsl_ba_schur_apply(self.h, C.byref(st), C.byref(o), x.ctypes.data_as(f64p), y.ctypes.data_as(f64p),
                                           C.c_int(nf)))
        return y

    def ba_schur_pcg(self, arr, b=None, tol=1e-8, max_iterations=None, use_huber=True, huber=1.0):
        """Solves S x = b (b None: g of ba_linearize) by the matrix-free block-Jacobi PCG (vsl_ba_schur_pcg).
        max_iterations None: 4 n.  Returns (x, iterations, rel_residual)."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        n = 6 * int((arr.cam_fixed == 0).sum())
        if b is not None:
            b = np.ascontiguousarray(b, np.float64).reshape(-1)
            if len(b) != n:
                raise ValueError("b has %d entries, the problem %d unknowns" % (len(b), n))
        x = np.zeros(n)
        it, rel = C.c_int(0), C.c_double(0.0)
        self._ck(self.L.vsl_ba_schur_pcg(self.h, C.byref(st), C.byref(o), None if b is None else b.ctypes.data_as(f64p),
                                         C.c_double(float(tol)), C.c_int(4 * n if max_iterations is None else int(max_iterations)),
                                         x.ctypes.data_as(f64p), C.byref(it), C.byref(rel)))
        return x, it.value, rel.value

    def ba_pcg_system(self, arr, inv_radius=0.0, b=None, v=None, tol=1e-8, max_iterations=None, use_huber=True, huber=1.0):
        """The Jacobi-scaled, damped reduced system of the iterative route's first LM step and one PCG solve on it, by
        the LM loop's own code (vsl_ba_pcg_system).  b None: the system's rhs; v: a vector for y = S' v (None: no
        product); max_iterations None: 4 n.  Returns a dict with scale_c, rhs, x, y (None without v) [n], Minv
        [n_free, 6, 6], cost and the record: status (1 converged, 2 numeric failure, 3 cap), iterations, pivot_fail, rr,
        bb, alpha, beta, segments (per camera), landmark_runs."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        nf = int((arr.cam_fixed == 0).sum())
        n = 6 * nf
        vec = {}
        for name, a in (("b", b), ("v", v)):
            if a is not None:
                a = np.ascontiguousarray(a, np.float64).reshape(-1)
                if len(a) != n:
                    raise ValueError("%s has %d entries, the problem %d unknowns" % (name, len(a), n))
            vec[name] = a
        scale_c, rhs, x, y, Minv = np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros((nf, 6, 6))
        cost, rec = C.c_double(), BaPcgRecord()
        ptr = lambda a: None if a is None else a.ctypes.data_as(f64p)
        self._ck(self.L.vsl_ba_pcg_system(self.h, C.byref(st), C.byref(o), C.c_double(float(inv_radius)), ptr(vec["b"]), ptr(vec["v"]),
                                          C.c_double(float(tol)), C.c_int(4 * n if max_iterations is None else int(max_iterations)),
                                          ptr(scale_c), ptr(rhs), C.byref(cost), ptr(Minv), ptr(x), ptr(y), C.byref(rec)))
        assert rec.n_free == nf
        return dict(scale_c=scale_c, rhs=rhs, cost=cost.value, Minv=Minv, x=x, y=None if v is None else y, status=rec.status,
                    iterations=rec.iterations, pivot_fail=rec.pivot_fail, rr=rec.rr, bb=rec.bb, alpha=rec.alpha, beta=rec.beta,
                    segments=rec.segments, landmark_runs=rec.landmark_runs)

    def last_ba_pcg(self):
        """(solves, iterations_total, iterations_last, rel_residual_last) of the matrix-free route in the last
        general-path bundle adjustment set up on this context; zeros when it did not take the route."""
        s, t, l, r = C.c_int64(), C.c_int64(), C.c_int(), C.c_double()
        self._ck(self.L.vsl_ctx_last_ba_pcg(self.h, C.byref(s), C.byref(t), C.byref(l), C.byref(r)))
        return s.value, t.value, l.value, r.value

    def ba_covariance(self, arr, cams=None, lms=None, use_huber=True, huber=1.0):
        """Marginal covariances at arr's poses / points (vsl_ba_covariance; nothing is optimised).  cams: camera ids
        (None: all free cameras), lms: landmark ids (None: none).  Returns (cov_pose [n, 6, 6], cov_point [m, 3, 3],
        n_degenerate); a landmark whose own block is singular comes back as NaN and is counted."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        cams = np.flatnonzero(arr.cam_fixed == 0) if cams is None else cams
        cams = np.ascontiguousarray(cams, np.int32).reshape(-1)
        lms = np.ascontiguousarray([] if lms is None else lms, np.int32).reshape(-1)
        cp, cl = np.zeros((len(cams), 6, 6)), np.zeros((len(lms), 3, 3))
        nd = C.c_int(0)
        self._ck(self.L.vsl_ba_covariance(self.h, C.byref(st), C.byref(o), cams.ctypes.data_as(i32p), len(cams),
                                          cp.ctypes.data_as(f64p), lms.ctypes.data_as(i32p), len(lms),
                                          cl.ctypes.data_as(f64p), C.byref(nd)))
        return cp, cl, nd.value

    def global_ba_covariance(self, arr, cams=None, lms=None, use_huber=True, huber=1.0):
        """ba_covariance for the map of a global bundle adjustment (vsl_global_ba_covariance): the same blocks, with the
        reduced camera system of a large map in band storage.  Returns (cov_pose [n, 6, 6], cov_point [m, 3, 3],
        n_degenerate, storage) with storage = 0 dense (the chain and the bits of ba_covariance) / 1 linear band."""
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        cams = np.flatnonzero(arr.cam_fixed == 0) if cams is None else cams
        cams = np.ascontiguousarray(cams, np.int32).reshape(-1)
        lms = np.ascontiguousarray([] if lms is None else lms, np.int32).reshape(-1)
        cp, cl = np.zeros((len(cams), 6, 6)), np.zeros((len(lms), 3, 3))
        nd, storage = C.c_int(0), C.c_int(-1)
        self._ck(self.L.vsl_global_ba_covariance(self.h, C.byref(st), C.byref(o), cams.ctypes.data_as(i32p), len(cams),
                                                 cp.ctypes.data_as(f64p), lms.ctypes.data_as(i32p), len(lms),
                                                 cl.ctypes.data_as(f64p), C.byref(nd), C.byref(storage)))
        return cp, cl, nd.value, storage.value

    def _ba_relpose(self, symbol, with_storage, arr, pairs, use_huber, huber):
        st = self._ba_struct(arr)
        o = self._ba_opts(use_huber, huber, 0, 0)
        pairs = np.asarray(pairs, np.int32).reshape(-1, 2)
        a, b = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        n = len(a)
        joint, meas, cov, info = np.zeros((n, 12, 12)), np.zeros((n, 6)), np.zeros((n, 6, 6)), np.zeros((n, 6, 6))
        ns, storage = C.c_int(0), C.c_int(-1)
        tail = (C.byref(storage),) if with_storage else ()
        self._ck(getattr(self.L, symbol)(self.h, C.byref(st), C.byref(o), a.ctypes.data_as(i32p), b.ctypes.data_as(i32p), n,
                                         joint.ctypes.data_as(f64p), meas.ctypes.data_as(f64p), cov.ctypes.data_as(f64p),
                                         info.ctypes.data_as(f64p), C.byref(ns), *tail))
        return (joint, meas, cov, info, ns.value) + ((storage.value,) if with_storage else ())

    def ba_relative_pose_covariance(self, arr, pairs, use_huber=True, huber=1.0):
        """Covariance and information of the relative poses of camera pairs under the bundle adjustment's posterior at
        arr's poses / points (vsl_ba_relative_pose_covariance, the dense route; nothing is optimised).  pairs: [n, 2]
        camera ids (a, b); one of the two may be fixed.  Returns (joint [n, 12, 12], meas [n, 6] = log(T_a^-1 T_b),
        cov [n, 6, 6] of the pose-graph residual, info [n, 6, 6] = cov^-1 (NaN where singular), n_singular): meas and
        info are edge_meas and edge_info of a pose graph, cov is meas_cov of pgo_edge_consistency."""
        return self._ba_relpose("vsl_ba_relative_pose_covariance", False, arr, pairs, use_huber, huber)

    def global_ba_relative_pose_covariance(self, arr, pairs, use_huber=True, huber=1.0):
        """ba_relative_pose_covariance for the map of a global bundle adjustment
        (vsl_global_ba_relative_pose_covariance).  Returns (joint, meas, cov, info, n_singular, storage) with storage =
        0 dense (the bits of ba_relative_pose_covariance) / 1 linear band."""
        return self._ba_relpose("vsl_global_ba_relative_pose_covariance", True, arr, pairs, use_huber, huber)

    def ba_residuals_jacobians(self, arr):
        st = self._ba_struct(arr)
        n = len(arr.obs_cam)
        r, Jp, Jl = np.zeros((n, 2)), np.zeros((n, 2, 6)), np.zeros((n, 2, 3))
        self._ck(self.L.vsl_ba_residuals_jacobians(self.h, C.byref(st), r.ctypes.data_as(f64p),
                                                   Jp.ctypes.data_as(f64p), Jl.ctypes.data_as(f64p)))
        return r, Jp, Jl

    # ---- DBoW2
    def load_vocabulary(self, path):
        return Vocabulary(self, path)

    def bow_score_batch(self, q_ids, q_vals, cands):
        """cands: list of (ids, vals).  Returns the L1 scores (float64 array)."""
        q_ids = np.ascontiguousarray(q_ids, np.uint32)
        q_vals = np.ascontiguousarray(q_vals, np.float64)
        m = len(cands)
        offs = np.zeros(m + 1, np.int32)
        for i, (ids, _) in enumerate(cands):
            offs[i + 1] = offs[i] + len(ids)
        c_ids = np.concatenate([np.asarray(c[0], np.uint32) for c in cands]) if m else np.zeros(0, np.uint32)
        c_vals = np.concatenate([np.asarray(c[1], np.float64) for c in cands]) if m else np.zeros(0)
        c_ids = np.ascontiguousarray(c_ids, np.uint32)
        c_vals = np.ascontiguousarray(c_vals, np.float64)
        scores = np.zeros(max(m, 1), np.float64)
        self._ck(self.L.vsl_bow_score_batch(self.h, q_ids.ctypes.data_as(u32p), q_vals.ctypes.data_as(f64p),
                                            len(q_ids), c_ids.ctypes.data_as(u32p),
                                            c_vals.ctypes.data_as(f64p), offs.ctypes.data_as(i32p), m,
                                            scores.ctypes.data_as(f64p)))
        return scores[:m].copy()


class BaArrays:
    """Owns the contiguous numpy arrays of a flattened bundle-adjustment problem (the layout of vsl_ba_problem,
    include/vslam_hip.h): what Context.bundle_adjust / ba_linearize and
    ba_dist.bundle_adjust_distributed take."""

    def __init__(self, poses, cam_fixed, cam_intr, intr, points, obs_cam, obs_lm, obs_uv, cam_model=(0, 0)):
        self.poses = np.ascontiguousarray(poses, np.float64).reshape(-1, 7).copy()
        self.cam_fixed = np.ascontiguousarray(cam_fixed, np.uint8).copy()
        self.cam_intr = np.ascontiguousarray(cam_intr, np.int32).copy()
        self.intr = np.ascontiguousarray(intr, np.float64).reshape(2, 8).copy()
        self.points = np.ascontiguousarray(points, np.float64).reshape(-1, 3).copy()
        self.obs_cam = np.ascontiguousarray(obs_cam, np.int32).copy()
        self.obs_lm = np.ascontiguousarray(obs_lm, np.int32).copy()
        self.obs_uv = np.ascontiguousarray(obs_uv, np.float64).reshape(-1, 2).copy()
        self.cam_model = tuple(int(m) for m in cam_model)

    @classmethod
    def from_dict(cls, d):
        return cls(d["poses"], d["cam_fixed"], d["cam_intr"], d["intr"], d["points"], d["obs_cam"], d["obs_lm"], d["obs_uv"],
                   d.get("cam_model", (0, 0)))

    def copy(self):
        return BaArrays(self.poses, self.cam_fixed, self.cam_intr, self.intr, self.points, self.obs_cam, self.obs_lm,
                        self.obs_uv, self.cam_model)

    @property
    def n_free(self):
        return int((self.cam_fixed == 0).sum())


class RigArrays:
    """Owns the contiguous numpy arrays of a vsl_ba_rig (include/vslam_hip.h): body poses [B, 7], body_fixed [B],
    cam_body [cameras of the BaArrays it goes with], T_b_c [2, 7]: what Context.bundle_adjust_rig / ba_rig_linearize /
    ba_rig_system take beside a BaArrays."""

    def __init__(self, body_poses, body_fixed, cam_body, T_b_c):
        self.body_poses = np.ascontiguousarray(body_poses, np.float64).reshape(-1, 7).copy()
        self.body_fixed = np.ascontiguousarray(body_fixed, np.uint8).copy()
        self.cam_body = np.ascontiguousarray(cam_body, np.int32).copy()
        self.T_b_c = np.ascontiguousarray(T_b_c, np.float64).reshape(2, 7).copy()

    def copy(self):
        return RigArrays(self.body_poses, self.body_fixed, self.cam_body, self.T_b_c)

    @property
    def n_free(self):
        return int((self.body_fixed == 0).sum())


class Vocabulary:
    def __init__(self, ctx, path):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._ck(ctx.L.vsl_voc_load_text(ctx.h, os.fsencode(str(path)), C.byref(h)))
        self.h = h

    def info(self):
        v = [C.c_int32() for _ in range(4)]
        self.ctx._ck(self.ctx.L.vsl_voc_info(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def transform(self, desc32, levelsup=4):
        desc32 = np.ascontiguousarray(desc32, np.uint8).reshape(-1, 32)
        n = len(desc32)
        ids = np.zeros(max(n, 1), np.uint32)
        vals = np.zeros(max(n, 1), np.float64)
        fn = np.zeros(max(n, 1), np.uint32)
        ff = np.zeros(max(n, 1), np.uint32)
        nnz, fvn = C.c_int32(), C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_bow_transform(self.ctx.h, self.h, desc32.ctypes.data_as(u8p), n,
                                                  int(levelsup), ids.ctypes.data_as(u32p),
                                                  vals.ctypes.data_as(f64p), C.byref(nnz),
                                                  fn.ctypes.data_as(u32p), ff.ctypes.data_as(u32p),
                                                  C.byref(fvn)))
        return (ids[:nnz.value].copy(), vals[:nnz.value].copy(), fn[:fvn.value].copy(),
                ff[:fvn.value].copy())

    def compute_bow_vector(self, img, num_features=1500, levelsup=4):
        """compute_bow_vector (keypoints.h:243-254): ORB front end + transform, one call.  An image with more features
        than the first buffers hold (ties are unbounded) is done once more with the count the call reports."""
        img, p, w, h, pitch = _img_rows(img)
        cap = 2 * num_features + 512
        for _ in range(2):
            ids = np.zeros(cap, np.uint32)
            vals = np.zeros(cap, np.float64)
            fn = np.zeros(cap, np.uint32)
            ff = np.zeros(cap, np.uint32)
            nnz, fvn = C.c_int32(), C.c_int32()
            rc = self.ctx.L.vsl_compute_bow_vector(self.ctx.h, self.h, p, w, h, pitch, int(num_features), int(levelsup), cap,
                                                   ids.ctypes.data_as(u32p), vals.ctypes.data_as(f64p), C.byref(nnz),
                                                   fn.ctypes.data_as(u32p), ff.ctypes.data_as(u32p), C.byref(fvn))
            if rc != -4 or fvn.value <= cap:   # VSL_ERR_CAPACITY: fvn = the capacity that suffices
                break
            cap = fvn.value
        self.ctx._ck(rc)
        return (ids[:nnz.value].copy(), vals[:nnz.value].copy(), fn[:fvn.value].copy(), ff[:fvn.value].copy())

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.vsl_voc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowDatabase:
    """Device-resident BowVectors (vsl_bowdb_*): append once per keyframe, score a query against any subset."""

    def __init__(self, ctx, cap_entries=1 << 20, cap_vectors=1024):
        self.ctx = ctx
        h = C.c_void_p()
        ctx._ck(ctx.L.vsl_bowdb_create(ctx.h, C.c_int64(int(cap_entries)), int(cap_vectors), C.byref(h)))
        self.h = h

    def append(self, ids, vals):
        ids = np.ascontiguousarray(ids, np.uint32)
        vals = np.ascontiguousarray(vals, np.float64)
        assert len(ids) == len(vals)
        idx = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_bowdb_append(self.ctx.h, self.h, ids.ctypes.data_as(u32p), vals.ctypes.data_as(f64p),
                                                 len(ids), C.byref(idx)))
        return idx.value

    def reserve(self, cap_entries, cap_vectors):
        """Room for cap_entries words and cap_vectors vectors in all (Frames.bow_vectors does not grow the database)."""
        self.ctx._ck(self.ctx.L.vsl_bowdb_reserve(self.ctx.h, self.h, C.c_int64(int(cap_entries)), int(cap_vectors)))

    def info(self):
        n, e = C.c_int32(), C.c_int64()
        self.ctx._ck(self.ctx.L.vsl_bowdb_info(self.h, C.byref(n), C.byref(e)))
        return n.value, e.value

    def score(self, q_ids, q_vals, cand_index=None, m=None):
        """L1 scores of the query against vectors cand_index (or the first m / all vectors)."""
        q_ids = np.ascontiguousarray(q_ids, np.uint32)
        q_vals = np.ascontiguousarray(q_vals, np.float64)
        if cand_index is not None:
            cand_index = np.ascontiguousarray(cand_index, np.int32)
            m = len(cand_index)
            ip = cand_index.ctypes.data_as(i32p)
        else:
            m = self.info()[0] if m is None else int(m)
            ip = None
        scores = np.zeros(max(m, 1), np.float64)
        self.ctx._ck(self.ctx.L.vsl_bowdb_score(self.ctx.h, self.h, q_ids.ctypes.data_as(u32p), q_vals.ctypes.data_as(f64p),
                                                len(q_ids), ip, m, scores.ctypes.data_as(f64p)))
        return scores[:m].copy()

    def query(self, q_ids, q_vals, n_words, exclude=(), keep_fraction=0.8, cap=None):
        """vsl_bowdb_query: the place-recognition vote, the keep_fraction rule and the L1 scores in one device pass.
        Returns (index, count, score, n_sharing, max_count); the candidates in ascending (first shared word, index)."""
        q_ids = np.ascontiguousarray(q_ids, np.uint32)
        q_vals = np.ascontiguousarray(q_vals, np.float64)
        assert len(q_ids) == len(q_vals)
        exclude = np.ascontiguousarray(exclude, np.int32)
        cap = self.info()[0] if cap is None else int(cap)
        idx = np.zeros(max(cap, 1), np.int32)
        cnt = np.zeros(max(cap, 1), np.int32)
        sc = np.zeros(max(cap, 1), np.float64)
        n, ns, mx = C.c_int32(), C.c_int32(), C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_bowdb_query(self.ctx.h, self.h, q_ids.ctypes.data_as(u32p), q_vals.ctypes.data_as(f64p),
                                                len(q_ids), C.c_uint32(int(n_words)), exclude.ctypes.data_as(i32p), len(exclude),
                                                C.c_float(float(keep_fraction)), cap, idx.ctypes.data_as(i32p),
                                                cnt.ctypes.data_as(i32p), sc.ctypes.data_as(f64p), C.byref(n), C.byref(ns),
                                                C.byref(mx)))
        return idx[:n.value].copy(), cnt[:n.value].copy(), sc[:n.value].copy(), ns.value, mx.value

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.vsl_bowdb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Event:
    """vsl_event: marks a point in one context's stream for another context to wait on (device side)."""

    def __init__(self, ctx):
        self.L = ctx.L
        h = C.c_void_p()
        ctx._ck(self.L.vsl_event_create(ctx.h, C.byref(h)))
        self.h = h

    def record(self, ctx):
        ctx._ck(self.L.vsl_event_record(self.h, ctx.h))

    def close(self):
        if getattr(self, "h", None):
            self.L.vsl_event_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Frames:
    """vsl_frames: device-resident batched frame store."""

    def __init__(self, ctx, max_images, w, h, max_features=1500, max_pairs=None):
        self.ctx = ctx
        self.max_images, self.w, self.hgt, self.F = max_images, w, h, max_features
        self.max_pairs = max_pairs if max_pairs is not None else max(1, max_images // 2)
        hnd = C.c_void_p()
        ctx._ck(ctx.L.vsl_frames_create(ctx.h, int(max_images), int(w), int(h), int(max_features),
                                        int(self.max_pairs), C.byref(hnd)))
        self.h = hnd

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.vsl_frames_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def images_dev(self):
        return self.ctx.L.vsl_frames_images_dev(self.h)

    def upload(self, first, imgs):
        imgs = np.ascontiguousarray(imgs, np.uint8)
        if imgs.ndim == 2:
            imgs = imgs[None]
        n, h, w = imgs.shape
        assert (h, w) == (self.hgt, self.w)
        self.ctx._ck(self.ctx.L.vsl_frames_upload(self.ctx.h, self.h, int(first), n,
                                                  imgs.ctypes.data_as(u8p), C.c_size_t(w),
                                                  C.c_size_t(w * h)))
        self.ctx.synchronize()

    def upload_async(self, first, imgs, ctx=None):
        """Enqueue the copy of a dense (n, h, w) uint8 batch -- pinned host memory for a truly asynchronous copy --
        on `ctx` (default: the store's own context) and return without waiting; the caller keeps `imgs` alive and
        unchanged until that stream has passed the copy."""
        c = ctx or self.ctx
        assert imgs.dtype == np.uint8 and imgs.ndim == 3 and imgs.flags["C_CONTIGUOUS"]
        n, h, w = imgs.shape
        assert (h, w) == (self.hgt, self.w)
        c._ck(c.L.vsl_frames_upload(c.h, self.h, int(first), n, imgs.ctypes.data_as(u8p), C.c_size_t(w),
                                    C.c_size_t(w * h)))

    def detect_describe(self, first, n, num_features=1500, rotate=True):
        self.ctx._ck(self.ctx.L.vsl_frames_detect_describe(self.ctx.h, self.h, int(first), int(n),
                                                           int(num_features), int(rotate)))

    def describe_at(self, first, corners, rotate=True, tie_rec_cap=4096):
        """Diagnostic (vsl_diag_frames_describe_at): describe the given integer corners -- one (k, 2) array per slot from
        `first` on -- and return (moments per slot as (k, 2) arrays of (m01, m10), raw near-tie word, tie records (m, 4))
        as the kernels left them; resolve_ties() / keypoints() finish the launch as after detect_describe."""
        corners = [np.ascontiguousarray(c, np.int32).reshape(-1, 2) for c in corners]
        n, cap = len(corners), max(1, max(len(c) for c in corners))
        xy = np.zeros((n, cap, 2), np.int32)
        for i, c in enumerate(corners):
            xy[i, :len(c)] = c
        counts = np.array([len(c) for c in corners], np.int32)
        mom = np.zeros((n, cap, 2), np.int32)
        rec = np.zeros((max(1, tie_rec_cap), 4), np.int32)
        nt = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_diag_frames_describe_at(self.ctx.h, self.h, int(first), n, xy.ctypes.data_as(i32p),
                                                            counts.ctypes.data_as(i32p), cap, int(rotate),
                                                            mom.ctypes.data_as(i32p), rec.ctypes.data_as(i32p),
                                                            int(tie_rec_cap), C.byref(nt)))
        n_rec = min(nt.value & ((1 << 30) - 1), tie_rec_cap)
        return [mom[i, :len(c)].copy() for i, c in enumerate(corners)], nt.value, rec[:n_rec].copy()

    def set_keypoints(self, first, descs, corners=None):
        """Diagnostic (vsl_diag_frames_set_keypoints): write descriptors -- one (k, 4) uint64 array per slot from `first`
        on -- and, with `corners` (one (k, 2) integer array per slot), corner positions straight into the store; a slot's
        keypoint count becomes its k.  Pending describe launches are resolved first."""
        descs = [np.ascontiguousarray(d, np.uint64).reshape(-1, 4) for d in descs]
        n, cap = len(descs), max([1] + [len(d) for d in descs])
        dd = np.zeros((max(n, 1), cap, 4), np.uint64)
        for i, d in enumerate(descs):
            dd[i, :len(d)] = d
        counts = np.array([len(d) for d in descs] or [0], np.int32)
        xy = None
        if corners is not None:
            corners = [np.ascontiguousarray(c, np.int32).reshape(-1, 2) for c in corners]
            assert [len(c) for c in corners] == [len(d) for d in descs]
            xy = np.zeros((max(n, 1), cap, 2), np.int32)
            for i, c in enumerate(corners):
                xy[i, :len(c)] = c
        self.ctx._ck(self.ctx.L.vsl_diag_frames_set_keypoints(self.ctx.h, self.h, int(first), n, counts.ctypes.data_as(i32p),
                                                              cap, xy.ctypes.data_as(i32p) if xy is not None else None,
                                                              dd.ctypes.data_as(u64p)))

    def resolve_ties(self):
        n = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_frames_resolve_ties(self.ctx.h, self.h, C.byref(n)))
        return n.value

    def exact_fallbacks(self):
        return int(self.ctx.L.vsl_frames_exact_fallbacks(self.h))

    def match(self, slot_pairs, threshold=70, dist_2_best=1.2):
        sp = np.ascontiguousarray(slot_pairs, np.int32).reshape(-1, 2)
        self.ctx._ck(self.ctx.L.vsl_frames_match(self.ctx.h, self.h, sp.ctypes.data_as(i32p), len(sp),
                                                 int(threshold), C.c_double(dist_2_best)))

    def keypoints(self, slot):
        xy = np.zeros((self.F, 2), np.float64)
        ang = np.zeros(self.F, np.float64)
        desc = np.zeros((self.F, 4), np.uint64)
        n = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_frames_download_keypoints(self.ctx.h, self.h, int(slot), self.F,
                                                              xy.ctypes.data_as(f64p),
                                                              ang.ctypes.data_as(f64p),
                                                              desc.ctypes.data_as(u64p), C.byref(n)))
        return xy[:n.value].copy(), ang[:n.value].copy(), desc[:n.value].copy()

    def matches(self, pair):
        out = np.zeros((self.F, 2), np.int32)
        n = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_frames_download_matches(self.ctx.h, self.h, int(pair), self.F,
                                                            out.ctypes.data_as(i32p), C.byref(n)))
        return out[:n.value].copy()

    def stereo_inliers(self, first_pair, n_pairs, cam_a, cam_b, E, R=None, t=None, threshold=1e-3, triangulate=True):
        """vsl_frames_stereo_inliers (asynchronous): epipolar inliers of the matches in pair slots
        [first_pair, first_pair + n_pairs) and, with R / t (R_0_1, t_0_1), their midpoint triangulation in the left
        camera's frame.  cam_a / cam_b = (VSL_CAM_* model, 8 intrinsics); E, R row-major 3 x 3."""
        E9, R9, t3 = _mat9(E), _mat9(R), _vec3(t)
        (ma, ia), (mb, ib) = _cam(cam_a), _cam(cam_b)
        self.ctx._ck(self.ctx.L.vsl_frames_stereo_inliers(
            self.ctx.h, self.h, int(first_pair), int(n_pairs), ma, ia.ctypes.data_as(f64p), mb, ib.ctypes.data_as(f64p),
            E9.ctypes.data_as(f64p), R9.ctypes.data_as(f64p) if R9 is not None else None,
            t3.ctypes.data_as(f64p) if t3 is not None else None, C.c_double(threshold), int(bool(triangulate))))

    def inliers(self, pair, points=True):
        """(pairs (n, 2) int32, points_c (n, 3) float64 or None) of one pair slot."""
        out = np.zeros((self.F, 2), np.int32)
        pts = np.zeros((self.F, 3), np.float64) if points else None
        n = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_frames_download_inliers(self.ctx.h, self.h, int(pair), self.F, out.ctypes.data_as(i32p),
                                                            pts.ctypes.data_as(f64p) if points else None, C.byref(n)))
        return out[:n.value].copy(), (pts[:n.value].copy() if points else None)

    def inlier_counts(self, n_pairs):
        c = np.zeros(max(n_pairs, 1), np.int32)
        self.ctx._ck(self.ctx.L.vsl_frames_download_inlier_counts(self.ctx.h, self.h, int(n_pairs), c.ctypes.data_as(i32p)))
        return c[:n_pairs].copy()

    def bow_vectors(self, first, n, voc, num_features=1500, levelsup=4, db=None, cap_per_image=None, host_outputs=True):
        """vsl_frames_bow_vectors: compute_bow_vector for the resident images [first, first + n) in one batched call.
        Returns a list of per-image (ids, vals, fv_node, fv_feat), exactly what Vocabulary.compute_bow_vector gives for
        each image; with `db` (a BowDatabase with room: BowDatabase.reserve) the vectors are also appended on the
        device and the result is (list, indices).  host_outputs=False downloads nothing (the list is None).  An image
        with more features than the first buffers hold is done once more with the count the call reports."""
        L, ctx = self.ctx.L, self.ctx
        n = int(n)
        cap = (2 * num_features + 512 if cap_per_image is None else int(cap_per_image)) if host_outputs else 0
        nfeat = np.zeros(max(n, 1), np.int32)
        index = np.zeros(max(n, 1), np.int32)
        for attempt in range(2):
            m = max(n * cap, 1)
            ids, vals = np.zeros(m, np.uint32), np.zeros(m, np.float64)
            fn, ff = np.zeros(m, np.uint32), np.zeros(m, np.uint32)
            nnz, fvn = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
            rc = L.vsl_frames_bow_vectors(ctx.h, self.h, int(first), n, voc.h if voc is not None else None, int(num_features),
                                          int(levelsup), db.h if db is not None else None, index.ctypes.data_as(i32p), cap,
                                          ids.ctypes.data_as(u32p), vals.ctypes.data_as(f64p), nnz.ctypes.data_as(i32p),
                                          fn.ctypes.data_as(u32p), ff.ctypes.data_as(u32p), fvn.ctypes.data_as(i32p),
                                          nfeat.ctypes.data_as(i32p))
            if rc != -4 or cap == 0 or cap_per_image is not None or nfeat[:n].max(initial=0) <= cap:
                break
            cap = int(nfeat[:n].max())   # VSL_ERR_CAPACITY: n_features = the capacities that suffice
        ctx._ck(rc)
        out = None
        if host_outputs:
            out = [(ids[i * cap:i * cap + nnz[i]].copy(), vals[i * cap:i * cap + nnz[i]].copy(),
                    fn[i * cap:i * cap + fvn[i]].copy(), ff[i * cap:i * cap + fvn[i]].copy()) for i in range(n)]
        return (out, index[:n].copy()) if db is not None else out

    def candidate_counts(self, n_images):
        nc = np.zeros(max(n_images, 1), np.int32)
        self.ctx._ck(self.ctx.L.vsl_frames_download_candidate_counts(self.ctx.h, self.h, int(n_images),
                                                                     nc.ctypes.data_as(i32p)))
        return nc[:n_images].copy()

    def response_max(self, n_images):
        mx = np.zeros(max(n_images, 1), np.float32)
        self.ctx._ck(self.ctx.L.vsl_frames_download_response_max(self.ctx.h, self.h, int(n_images),
                                                                 mx.ctypes.data_as(C.POINTER(C.c_float))))
        return mx[:n_images].copy()

    def counts(self, n_images, n_pairs):
        nk = np.zeros(max(n_images, 1), np.int32)
        nm = np.zeros(max(n_pairs, 1), np.int32)
        self.ctx._ck(self.ctx.L.vsl_frames_download_counts(self.ctx.h, self.h, int(n_images),
                                                           nk.ctypes.data_as(i32p), int(n_pairs),
                                                           nm.ctypes.data_as(i32p)))
        return nk[:n_images].copy(), nm[:n_pairs].copy()


class Map:
    """vsl_map: device-resident landmark table + observation-descriptor pool (per-frame tracking)."""

    def __init__(self, ctx, cap_landmarks=4096, cap_descriptors=16384):
        self.ctx = ctx
        hnd = C.c_void_p()
        ctx._ck(ctx.L.vsl_map_create(ctx.h, int(cap_landmarks), int(cap_descriptors), C.byref(hnd)))
        self.h = hnd

    def close(self):
        if getattr(self, "h", None):
            self.ctx.L.vsl_map_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def append_descriptors(self, desc):
        desc = np.ascontiguousarray(desc, np.uint64).reshape(-1, 4)
        first = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_map_append_descriptors(self.h, len(desc), desc.ctypes.data_as(u64p), C.byref(first)))
        return first.value

    def append_descriptors_from_frame(self, frames, slot, feature_ids):
        ids = np.ascontiguousarray(feature_ids, np.int32)
        first = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_map_append_descriptors_from_frame(self.h, frames.h, int(slot), len(ids),
                                                                      ids.ctypes.data_as(i32p), C.byref(first)))
        return first.value

    def set_landmarks(self, points, obs_start, obs_pool_index):
        points = np.ascontiguousarray(points, np.float64).reshape(-1, 3)
        obs_start = np.ascontiguousarray(obs_start, np.int32)
        obs_pool_index = np.ascontiguousarray(obs_pool_index, np.int32)
        self.ctx._ck(self.ctx.L.vsl_map_set_landmarks(self.h, len(points), points.ctypes.data_as(f64p),
                                                      obs_start.ctypes.data_as(i32p), obs_pool_index.ctypes.data_as(i32p)))

    def info(self):
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_map_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def track(self, frames, slot, pose7, model, intr8, width, height, cam_z_threshold=0.1, max_dist_2d=20.0, threshold=70,
              dist_2_best=1.2, with_corners=False):
        """project_landmarks + find_matches_landmarks against the frame store slot: (pairs, n_projected); with_corners:
        also the slot's keypoint positions from the same round trip (vsl_map_track_corners)."""
        pose7 = np.ascontiguousarray(pose7, np.float64)
        intr8 = np.ascontiguousarray(intr8, np.float64)
        pairs = np.zeros((frames.F, 2), np.int32)
        n, npj = C.c_int32(), C.c_int32()
        if not with_corners:
            self.ctx._ck(self.ctx.L.vsl_map_track(self.h, frames.h, int(slot), pose7.ctypes.data_as(f64p), int(model),
                                                  intr8.ctypes.data_as(f64p), int(width), int(height), C.c_double(cam_z_threshold),
                                                  C.c_double(max_dist_2d), int(threshold), C.c_double(dist_2_best),
                                                  pairs.ctypes.data_as(i32p), C.byref(n), C.byref(npj)))
            return pairs[:n.value].copy(), npj.value
        xy = np.zeros((frames.F, 2), np.float64)
        nk = C.c_int32()
        self.ctx._ck(self.ctx.L.vsl_map_track_corners(self.h, frames.h, int(slot), pose7.ctypes.data_as(f64p), int(model),
                                                      intr8.ctypes.data_as(f64p), int(width), int(height),
                                                      C.c_double(cam_z_threshold), C.c_double(max_dist_2d), int(threshold),
                                                      C.c_double(dist_2_best), pairs.ctypes.data_as(i32p), C.byref(n),
                                                      C.byref(npj), xy.ctypes.data_as(f64p), C.byref(nk)))
        return pairs[:n.value].copy(), npj.value, xy[:nk.value].copy()
