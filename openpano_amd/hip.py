"""ctypes binding of ``libopenpano_hip.so`` (the C-ABI in ``include/openpano_hip.h``).

There is deliberately no fallback: if the HIP library is missing or no gfx950 device is
present, loading / creating a context raises.  Device buffers can be handed over as raw
pointers (e.g. ``torch.Tensor.data_ptr()``), PyTorch is never imported here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OPENPANO_HIP_LIB") or os.path.join(_HERE, "libopenpano_hip.so")     # override: A/B builds of the same ABI (scripts/)


class OpenPanoHipError(RuntimeError):
    pass


class OpConfig(C.Structure):
    """``op_config`` (include/openpano_hip.h), POD snapshot of ``namespace config``."""
    _fields_ = [
        ("SIFT_WORKING_SIZE", C.c_int), ("NUM_OCTAVE", C.c_int), ("NUM_SCALE", C.c_int),
        ("SCALE_FACTOR", C.c_float), ("GAUSS_SIGMA", C.c_float), ("GAUSS_WINDOW_FACTOR", C.c_int),
        ("JUDGE_EXTREMA_DIFF_THRES", C.c_float), ("CONTRAST_THRES", C.c_float),
        ("PRE_COLOR_THRES", C.c_float), ("EDGE_RATIO", C.c_float),
        ("CALC_OFFSET_DEPTH", C.c_int), ("OFFSET_THRES", C.c_float),
        ("ORI_RADIUS", C.c_float), ("ORI_HIST_SMOOTH_COUNT", C.c_int),
        ("DESC_HIST_SCALE_FACTOR", C.c_int), ("DESC_INT_FACTOR", C.c_int),
        ("MATCH_REJECT_NEXT_RATIO", C.c_float), ("RANSAC_ITERATIONS", C.c_int),
        ("RANSAC_INLIER_THRES", C.c_double),
        ("INLIER_IN_MATCH_RATIO", C.c_float), ("INLIER_IN_POINTS_RATIO", C.c_float),
        ("CYLINDER", C.c_int), ("TRANS", C.c_int), ("ESTIMATE_CAMERA", C.c_int),
        ("ORDERED_INPUT", C.c_int), ("LAZY_READ", C.c_int), ("MULTIBAND", C.c_int),
        ("MAX_OUTPUT_SIZE", C.c_int), ("FOCAL_LENGTH", C.c_float),
    ]

    @classmethod
    def from_config(cls, cfg):
        c = cls()
        for name, _ in cls._fields_:
            setattr(c, name, getattr(cfg, name))
        return c


class OpImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("on_device", C.c_int), ("dtype", C.c_int)]


OP_F32, OP_U8 = 0, 1
OP_SRC_DEVICE, OP_SRC_U8 = 1, 2        # bits of op_blend_image.on_device


class OpBlendImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("h", C.c_int), ("w", C.c_int), ("on_device", C.c_int),
                ("homo_inv", C.c_double * 9), ("range", C.c_double * 4), ("mat_h", C.c_int), ("mat_w", C.c_int)]


class OpBlendGeom(C.Structure):
    _fields_ = [("proj_method", C.c_int), ("proj_min", C.c_double * 2), ("proj_max", C.c_double * 2),
                ("resolution", C.c_double * 2)]


class OpPanoFrame(C.Structure):
    """``op_pano_frame``: where an equirectangular canvas sits on the sphere (column c at longitude lon0 + c * step_lon, row r at
    latitude lat0 + r * step_lat; wrap = 1: the columns span exactly one turn)"""
    _fields_ = [("lon0", C.c_double), ("lat0", C.c_double), ("step_lon", C.c_double), ("step_lat", C.c_double), ("wrap", C.c_int)]


class OpViewSpec(C.Structure):
    """``op_view_spec``: what ``Canvas.reproject`` makes (mode: VIEW_PLANET or VIEW_RECTILINEAR)"""
    _fields_ = [("mode", C.c_int), ("out_h", C.c_int), ("out_w", C.c_int), ("rot", C.c_double * 9), ("focal", C.c_double)]


VIEW_PLANET, VIEW_RECTILINEAR = 0, 1      # OP_VIEW_PLANET, OP_VIEW_RECTILINEAR


# The prototypes of include/openpano_hip.h, in the header's order: name -> (restype, argtypes).  lib() binds exactly these and
# refuses a library that lacks one; tests/test_binding_header_cpu.py holds the table against the header.  Handles and array
# arguments are c_void_p (see _p), out-parameters for scalars and the structs are typed pointers.
_V, _S, _I, _I64, _U32, _F, _D = C.c_void_p, C.c_char_p, C.c_int, C.c_int64, C.c_uint32, C.c_float, C.c_double
_PV, _PS, _PI, _PI64 = C.POINTER(_V), C.POINTER(_S), C.POINTER(_I), C.POINTER(_I64)
_CFG, _IMG, _BIMG, _GEOM = C.POINTER(OpConfig), C.POINTER(OpImage), C.POINTER(OpBlendImage), C.POINTER(OpBlendGeom)
_FRAME, _SPEC = C.POINTER(OpPanoFrame), C.POINTER(OpViewSpec)
_BLEND = [_V, _CFG, _GEOM, _BIMG, _I]        # ctx, cfg, geometry, images, n: how every blend and overlap call starts
_RANSAC = [_V, _CFG, _V, _V, _V, _I, _V, _V, _U32, _PV]

PROTOTYPES = {
    "op_last_error": (_S, []),
    "op_abi_version": (_I, []),
    # configuration
    "op_config_default": (None, [_CFG]),
    # context
    "op_ctx_create": (_I, [_I, _V, _PV]),
    "op_ctx_destroy": (None, [_V]),
    "op_ctx_sync": (_I, [_V]),
    "op_ctx_set_profiling": (_I, [_V, _I]),
    "op_ctx_profile_only": (_I, [_V, _S]),
    "op_ctx_profile_reset": (_I, [_V]),
    "op_ctx_profile_count": (_I, [_V]),
    "op_ctx_profile_get": (_I, [_V, _I, _PS, C.POINTER(_D), C.POINTER(C.c_long)]),
    # SIFT
    "op_sift_batch": (_I, [_V, _CFG, _IMG, _I, _PV]),
    "op_sift_batch_host": (_I, [_V, _CFG, _IMG, _I, _V, _V, _I64, _PV]),
    "op_features_num_images": (_I, [_V]),
    "op_features_count": (_I, [_V, _I]),
    "op_features_offset": (_I64, [_V, _I]),
    "op_features_total": (_I64, [_V]),
    "op_features_desc_device": (_V, [_V]),
    "op_features_coor_device": (_V, [_V]),
    "op_features_copy": (_I, [_V, _V, _I, _V, _V]),
    "op_features_copy_real": (_I, [_V, _V, _I, _V]),
    "op_features_from_host": (_I, [_V, _PV, _PV, _PI, _I, _PV]),
    "op_features_from_device": (_I, [_V, _V, _V, _PI, _I, _PV]),
    "op_features_adopt_device": (_I, [_V, _V, _V, _PI, _I, _PV]),
    "op_features_free": (None, [_V]),
    # staged single-image run
    "op_sift_staged": (_I, [_V, _CFG, _IMG, _PV]),
    "op_sift_dump_free": (None, [_V]),
    "op_sift_dump_working_dims": (_I, [_V, _PI, _PI]),
    "op_sift_dump_octave_dims": (_I, [_V, _I, _PI, _PI]),
    "op_sift_dump_plane": (_I, [_V, _V, _I, _I, _I, _V]),
    "op_sift_dump_raw_count": (_I, [_V, _I, _I]),
    "op_sift_dump_raw": (_I, [_V, _I, _I, _V]),
    "op_sift_dump_kp_count": (_I, [_V, _I]),
    "op_sift_dump_kp": (_I, [_V, _I, _V, _V, _V]),
    "op_sift_dump_desc": (_I, [_V, _V, _V]),
    # test hooks
    "op_debug_math": (_I, [_V, _I, _V, _V, _I, _V]),
    "op_debug_set_raw_capacity": (_I, [_V, _I]),
    "op_debug_set_desc_list_cap": (_I, [_V, _I]),
    "op_debug_pool_stats": (_I, [_PI64, _PI64, _PI64]),
    "op_debug_match_last_slow": (_I, [_V, _PI, _PI]),
    # match
    "op_match_pairs": (_I, [_V, _CFG, _V, _V, _I, _PV]),
    "op_matches_count": (_I, [_V, _I]),
    "op_matches_copy": (_I, [_V, _I, _V]),
    "op_matches_copy_all": (_I, [_V, _V, _V]),
    "op_matches_device_list": (_V, [_V]),
    "op_matches_total": (_I64, [_V]),
    "op_matches_from_host": (_I, [_PV, _PI, _I, _PV]),
    "op_matches_concat": (_I, [_V, _V, _V, _PV]),
    "op_matches_free": (None, [_V]),
    # several GPUs in one process
    "op_group_create": (_I, [_PI, _I, _PV]),
    "op_group_destroy": (None, [_V]),
    "op_group_size": (_I, [_V]),
    "op_group_ctx": (_V, [_V, _I]),
    "op_sift_batch_multi": (_I, [_V, _CFG, _IMG, _I, _PV]),
    "op_match_pairs_multi": (_I, [_V, _CFG, _V, _V, _I, _PV]),
    "op_ransac_pairs_multi": (_I, _RANSAC),
    # RANSAC
    "op_ransac_pairs": (_I, _RANSAC),
    "op_ransac_ok": (_I, [_V, _I]),
    "op_ransac_confidence": (_F, [_V, _I]),
    "op_ransac_homo": (_I, [_V, _I, _V]),
    "op_ransac_inlier_count": (_I, [_V, _I]),
    "op_ransac_inliers": (_I, [_V, _I, _V]),
    "op_ransac_best": (_I, [_V, _I, _PI, _PI]),
    "op_ransac_summary": (_I, [_V, _PI, _PI64]),
    "op_ransac_free": (None, [_V]),
    "op_pairwise_table_size": (_I, [_V, _PI, _PI64]),
    "op_pairwise_table": (_I, [_V, _V, _V, _V, _V, _I, _V, _V, _V, _V, _V]),
    # warp + blend
    "op_blend_prepare": (_I, [_CFG, _I, _I, _I, _V, _V, _GEOM, _V, _V]),
    "op_blend_canvas_dims": (_I, [_GEOM, _BIMG, _I, _PI, _PI]),
    "op_blend": (_I, _BLEND + [_PV]),
    "op_canvas_dims": (_I, [_V, _PI, _PI]),
    "op_canvas_device": (_V, [_V]),
    "op_canvas_copy": (_I, [_V, _V, _V]),
    "op_canvas_free": (None, [_V]),
    "op_canvas_crop": (_I, [_V, _V, _PV, _PI, _PI]),
    "op_canvas_copy_u8": (_I, [_V, _V, _V]),
    # exposure (gain) compensation
    "op_gain_overlap": (_I, _BLEND + [_I, _V, _V]),
    "op_gain_solve": (_I, [_I, _V, _V, _D, _D, _I, _V]),
    "op_blend_gains": (_I, _BLEND + [_V, _PV]),
    # block gain compensation
    "op_gain_block_overlap": (_I, _BLEND + [_I, _I, _I, _V, _V]),
    "op_gain_block_solve": (_I, [_I, _I, _I, _V, _V, _D, _D, _D, _I, _V]),
    "op_blend_block_gains": (_I, _BLEND + [_I, _I, _V, _PV]),
    # vignetting compensation
    "op_vignette_overlap": (_I, _BLEND + [_I, _F, _V, _V]),
    "op_vignette_solve": (_I, [_I, _V, _V, _I, _D, _D, _D, _V, _V]),
    "op_blend_vignette": (_I, _BLEND + [_V, _V, _PV]),
    # PNG output
    "op_canvas_encode_png": (_I, [_V, _V, _PV]),
    "op_png_encode_u8": (_I, [_V, _V, _I, _I, _PV]),
    "op_png_size": (_I64, [_V]),
    "op_png_copy": (_I, [_V, _V, _V]),
    "op_png_free": (None, [_V]),
    # JPEG output
    "op_canvas_encode_jpeg": (_I, [_V, _V, _I, _I, _PV]),
    "op_jpeg_encode_u8": (_I, [_V, _V, _I, _I, _I, _I, _PV]),
    "op_jpeg_size": (_I64, [_V]),
    "op_jpeg_copy": (_I, [_V, _V, _V]),
    "op_jpeg_free": (None, [_V]),
    # CYLINDER mode: pre-warp, perspective correction
    "op_cyl_warp_shape": (_I, [_CFG, _I, _I, _D, _V, _I, _PI, _PI, _V]),
    "op_cyl_warp": (_I, [_V, _CFG, _IMG, _D, _PV]),
    "op_canvas_upload": (_I, [_V, _V, _I, _I, _PV]),
    "op_perspective_homography": (_I, [_GEOM, _I, _I, _I, _I, _V, _I, _I, _V, _I, _I, _V, _V]),
    "op_canvas_perspective": (_I, [_V, _CFG, _V, _V, _PV]),
    # resident views
    "op_views_upload": (_I, [_V, _IMG, _I, _PV]),
    "op_views_count": (_I, [_V]),
    "op_views_image": (_I, [_V, _I, _IMG]),
    "op_views_blend_image": (_I, [_V, _I, _BIMG]),
    "op_views_free": (None, [_V]),
    # JPEG input (files travel as bytes: c_char_p)
    "op_jpeg_probe": (_I, [_S, _I64, _PI, _PI, _PI]),
    "op_views_decode_jpeg": (_I, [_V, _PS, _PI64, _I, _PV]),
    "op_views_copy": (_I, [_V, _V, _I, _V]),
    "op_debug_set_jpeg_subseq_bits": (_I, [_V, _I]),
    "op_debug_jpeg_last_rounds": (_I, [_V]),
    # EXIF orientation
    "op_jpeg_exif": (_I, [_S, _I64, _PI, _PI]),
    "op_views_decode_jpeg_oriented": (_I, [_V, _PS, _PI64, _I, _PI, _PV]),
    # re-projection of a finished panorama
    "op_pano_frame_of": (_I, [_GEOM, _I, _I, _FRAME]),
    "op_view_look": (_I, [_D, _D, _D, _D, _I, _I, _SPEC]),
    "op_view_cube_face": (_I, [_I, _I, _SPEC]),
    "op_view_planet": (_I, [_I, _SPEC]),
    "op_canvas_reproject": (_I, [_V, _V, _FRAME, _SPEC, _PV]),
}

_lib = None


def _bind_torch_hip_runtime():
    """Share ONE HIP runtime with PyTorch.

    The PyTorch ROCm wheel bundles its own ``libamdhip64.so`` (same SONAME as /opt/rocm's).  Two
    runtime instances in one process cannot see each other's allocations or streams (and the
    second one finds no GPU), so when torch is installed its copy is loaded first -- by path,
    without importing torch -- and ``libopenpano_hip.so`` then resolves ``libamdhip64.so.7`` to
    it.  Without torch (plain C++ hosts) the system ROCm runtime is used.
    """
    import importlib.util
    import sys
    if os.environ.get("OPENPANO_SYSTEM_HIP"):
        return
    try:
        spec = sys.modules["torch"].__spec__ if "torch" in sys.modules else importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        C.CDLL(cand, mode=os.RTLD_NOW | os.RTLD_GLOBAL)


def lib():
    """Load the HIP library (once). Raises if it has not been built -- no CPU fallback -- or lacks an entry point of PROTOTYPES."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise OpenPanoHipError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C openpano_amd/csrc`; openpano_amd has no CPU fallback")
    _bind_torch_hip_runtime()
    L = C.CDLL(LIB_PATH)
    missing = []
    for name, (restype, argtypes) in PROTOTYPES.items():
        try:
            fn = getattr(L, name)
        except AttributeError:
            missing.append(name)
            continue
        fn.restype, fn.argtypes = restype, argtypes
    if missing:
        raise OpenPanoHipError(f"{LIB_PATH} does not export {', '.join(missing)}: it was built from another include/openpano_hip.h")
    _lib = L
    return L


def use_library(path):
    """Switch this process to another build of the same ABI (the A/B scripts) -> lib().  Close every context and free every
    handle of the previous library first."""
    global _lib, LIB_PATH
    LIB_PATH = path
    _lib = None
    return lib()


def check(rc):
    if rc != 0:
        raise OpenPanoHipError(f"libopenpano_hip error {rc}: {lib().op_last_error().decode(errors='replace')}")


def _p(a):
    """a numpy array's data as the c_void_p the table declares for array arguments; None -> NULL"""
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _pairs(a):
    """(n, 2) contiguous int32: a list of image pairs (i, j)"""
    return np.ascontiguousarray(np.asarray(a, np.int32).reshape(-1, 2))


_shapes = _pairs        # (n, 2) contiguous int32 just the same: the images' (w, h)


def _seeds(seeds):
    """per-pair RANSAC seeds as contiguous uint32, or None (the library derives them from base_seed)"""
    return None if seeds is None else np.ascontiguousarray(np.asarray(seeds, np.uint32))


def _cfg(cfg):
    """a config object as the ``const op_config*`` argument of one call"""
    return C.byref(OpConfig.from_config(cfg))


def _new(fn, *args):
    """fn(*args, &handle), checked -> the handle the library made"""
    h = C.c_void_p()
    check(fn(*args, C.byref(h)))
    return h


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)


class _Handle:
    """Owner of one library object: ``handle`` is its pointer, None once freed (the object is then false); ``_free_fn`` names
    the entry point that releases it."""
    _free_fn = None
    handle = None

    def free(self):
        if self.handle:
            getattr(lib(), self._free_fn)(self.handle)
            self.handle = None

    def __bool__(self):
        return bool(self.handle)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pool_stats():
    """test hook: (live_blocks, live_bytes, cached_bytes) of the process-wide device pool (op_debug_pool_stats)"""
    v = [C.c_int64(), C.c_int64(), C.c_int64()]
    check(lib().op_debug_pool_stats(*(C.byref(x) for x in v)))
    return tuple(x.value for x in v)


class Context(_Handle):
    """``op_ctx``: one per (process, device); ``stream`` is an optional raw ``hipStream_t``."""
    _free_fn = "op_ctx_destroy"

    def __init__(self, device: int = 0, stream: int | None = None):
        self.handle = _new(lib().op_ctx_create, device, C.c_void_p(stream) if stream else None)
        self.device = device

    def sync(self):
        check(lib().op_ctx_sync(self.handle))

    def set_profiling(self, enable=True, only=None):
        """per-stage HIP-event timing on this context's stream; only = one stage label to bracket (None: all)"""
        check(lib().op_ctx_profile_only(self.handle, only.encode() if only else None))
        check(lib().op_ctx_set_profiling(self.handle, int(enable)))

    def profile_reset(self):
        check(lib().op_ctx_profile_reset(self.handle))

    def profile(self):
        """{stage label: (total_ms, calls)} measured with HIP events on this context's stream"""
        out = {}
        for i in range(lib().op_ctx_profile_count(self.handle)):
            lab = C.c_char_p(); ms = C.c_double(); calls = C.c_long()
            check(lib().op_ctx_profile_get(self.handle, i, C.byref(lab), C.byref(ms), C.byref(calls)))
            out[lab.value.decode()] = (ms.value, calls.value)
        return out

    def set_desc_list_cap(self, floats: int):
        """test hook: list arena one sorting pass of the descriptor kernel may use (op_debug_set_desc_list_cap)"""
        check(lib().op_debug_set_desc_list_cap(self.handle, int(floats)))

    def set_jpeg_subseq_bits(self, bits: int):
        """test hook: bits of a subsequence of the JPEG decoder's parallel Huffman decode, a multiple of 32; 0 = the default
        (op_debug_set_jpeg_subseq_bits)"""
        check(lib().op_debug_set_jpeg_subseq_bits(self.handle, int(bits)))

    def jpeg_last_rounds(self) -> int:
        """test hook: synchronisation rounds of the last Views.decode_jpeg on this context (op_debug_jpeg_last_rounds)"""
        return lib().op_debug_jpeg_last_rounds(self.handle)

    def match_last_slow(self):
        """test hook: (forward, reverse) rows the last match_pairs call on this context queued for the exact full scan, (-1, -1)
        before the first (op_debug_match_last_slow)"""
        f, r = C.c_int(), C.c_int()
        check(lib().op_debug_match_last_slow(self.handle, C.byref(f), C.byref(r)))
        return f.value, r.value

    def set_raw_capacity(self, cap: int):
        """test hook: per-image capacity of the speculative raw / refined lists (op_debug_set_raw_capacity)"""
        check(lib().op_debug_set_raw_capacity(self.handle, int(cap)))

    def close(self):
        self.free()


class _BorrowedContext(Context):
    """a context owned by an op_group (never destroyed from Python)"""

    def __init__(self, handle, device):
        self.handle = C.c_void_p(handle)
        self.device = device

    def free(self):
        self.handle = None


class Group(_Handle):
    """``op_group``: several GPUs driven from this process; a device may be listed twice."""
    _free_fn = "op_group_destroy"

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        self.handle = _new(lib().op_group_create, devs, len(devices))
        self.devices = list(devices)
        self.ctx0 = _BorrowedContext(lib().op_group_ctx(self.handle, 0), devices[0])

    def sift_batch(self, cfg, images) -> "Features":
        arr, keep = _mk_images(images)
        h = _new(lib().op_sift_batch_multi, self.handle, _cfg(cfg), arr, len(images))
        del keep
        return Features(self.ctx0, h)

    def match_pairs_handle(self, cfg, feats, pairs) -> "Matches":
        return _match(self, cfg, feats, pairs)

    def ransac_pairs(self, cfg, feats, matches, pairs, shapes_wh, seeds=None, base_seed=0):
        """op_ransac_pairs_multi -> the same list of dicts as hip.ransac_pairs"""
        return ransac_pairs(self, cfg, feats, matches, pairs, shapes_wh, seeds, base_seed)

    def free(self):
        if self.handle:
            self.ctx0.free()
        super().free()

    def close(self):
        self.free()


def _mk_images(images):
    """images: numpy HWC arrays (float32 in [0,1], or uint8 decoder bytes), or device buffers as
    (device_ptr, h, w) / (device_ptr, h, w, "u8") tuples."""
    arr = (OpImage * len(images))()
    keep = []
    for i, im in enumerate(images):
        if isinstance(im, tuple):
            ptr, h, w = im[:3]
            dt = OP_U8 if len(im) > 3 and im[3] in ("u8", OP_U8, np.uint8) else OP_F32
            arr[i] = OpImage(C.c_void_p(int(ptr)), int(h), int(w), 1, dt)
        else:
            im = np.asarray(im)
            a = np.ascontiguousarray(im) if im.dtype == np.uint8 else np.ascontiguousarray(im, np.float32)
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("image must be H x W x 3 (float32 or uint8)")
            keep.append(a)
            arr[i] = OpImage(_p(a), a.shape[0], a.shape[1], 0, OP_U8 if a.dtype == np.uint8 else OP_F32)
    return arr, keep


class Views(_Handle):
    """``op_views``: the views of a job uploaded once, each in the type it arrived in (float32, or uint8 decoder bytes),
    resident for ``sift_batch`` / ``cyl_warp`` (``images()``) and for ``blend`` and the overlap passes (pass the object, or
    ``blend_images()``).  The seam of ImageRef::load / img (stitch/imageref.hh:15-31)."""
    _free_fn = "op_views_free"

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.handle = handle

    @classmethod
    def upload(cls, ctx: Context, images) -> "Views":
        """images: as ``sift_batch`` takes them (numpy HWC float32 / uint8, or device tuples); one copy for a
        contiguous stack of host frames"""
        arr, keep = _mk_images(images)
        h = _new(lib().op_views_upload, ctx.handle, arr, len(images))
        del keep
        return cls(ctx, h)

    @classmethod
    def decode_jpeg(cls, ctx: Context, files, orient=False) -> "Views":
        """files: a list of baseline JPEG files as bytes; decoded on the device into uint8 views that equal libjpeg's
        default decode byte for byte (op_views_decode_jpeg).  All or nothing: a file outside the format or a corrupt one
        raises, naming its index.
        orient: False: the pixels as stored.  True: every view turned upright by its file's EXIF orientation.  A sequence
        of ints, one per file: 1..8 used as given, 0 = the file's EXIF (op_views_decode_jpeg_oriented)."""
        files = [bytes(f) for f in files]
        arr = (C.c_char_p * len(files))(*files)
        sizes = (C.c_int64 * len(files))(*[len(f) for f in files])
        if orient is False:
            return cls(ctx, _new(lib().op_views_decode_jpeg, ctx.handle, arr, sizes, len(files)))
        if orient is True:
            how = None
        else:
            orient = [int(o) for o in orient]
            if len(orient) != len(files):
                raise ValueError("orient: one orientation per file")
            how = (C.c_int * len(files))(*orient)
        return cls(ctx, _new(lib().op_views_decode_jpeg_oriented, ctx.handle, arr, sizes, len(files), how))

    def numpy(self, i: int) -> np.ndarray:
        """view i read back as (H, W, 3) in its own type, uint8 or float32 (op_views_copy)"""
        im = OpImage()
        check(lib().op_views_image(self.handle, int(i), C.byref(im)))
        out = np.empty((im.h, im.w, 3), np.uint8 if im.dtype == OP_U8 else np.float32)
        check(lib().op_views_copy(self.ctx.handle, self.handle, int(i), _p(out)))
        return out

    @property
    def count(self):
        return lib().op_views_count(self.handle)

    def __len__(self):
        return self.count

    def images(self):
        """device tuples (ptr, h, w[, "u8"]) for sift_batch / cyl_warp; valid until free()"""
        out = []
        for i in range(self.count):
            im = OpImage()
            check(lib().op_views_image(self.handle, i, C.byref(im)))
            out.append((im.data, im.h, im.w, "u8") if im.dtype == OP_U8 else (im.data, im.h, im.w))
        return out

    def blend_images(self):
        """an ``op_blend_image`` array with data, h, w and the source flags filled (homo_inv / range zero)"""
        arr = (OpBlendImage * self.count)()
        for i in range(self.count):
            check(lib().op_views_blend_image(self.handle, i, C.byref(arr[i])))
        return arr


JPEG_SAMPLING_NAMES = {0: "444", 1: "420", 2: "422", 3: "grey"}


def jpeg_probe(data):
    """(h, w, sampling) of a JPEG file that ``Views.decode_jpeg`` accepts, sampling one of "444", "422", "420", "grey";
    raises OpenPanoHipError (error -4: outside the format, -1: broken) otherwise.  Host only: needs no device."""
    data = bytes(data)
    h, w, s = C.c_int(), C.c_int(), C.c_int()
    check(lib().op_jpeg_probe(data, len(data), C.byref(h), C.byref(w), C.byref(s)))
    return h.value, w.value, JPEG_SAMPLING_NAMES[s.value]


def jpeg_exif(data):
    """(orientation, focal35) of a JPEG file's EXIF block: orientation 1..8 (1 when absent or unreadable) and
    FocalLengthIn35mmFilm in mm (0 when absent).  Malformed EXIF is no error; only a file without SOI raises.
    Host only: needs no device (op_jpeg_exif)."""
    data = bytes(data)
    o, f = C.c_int(), C.c_int()
    check(lib().op_jpeg_exif(data, len(data), C.byref(o), C.byref(f)))
    return o.value, f.value


def _mk_blend_images(images):
    """the sources of a blend as an ``op_blend_image`` array (data, h, w, flag word): a ``Views``, or a list of numpy HWC
    arrays (float32, or uint8 decoder bytes: OP_SRC_U8) and device tuples (ptr, h, w) / (ptr, h, w, "u8")"""
    if isinstance(images, Views):
        return images.blend_images(), images
    arr_img, keep = _mk_images(images)
    arr = (OpBlendImage * len(images))()
    for i in range(len(images)):
        arr[i].data = arr_img[i].data; arr[i].h = arr_img[i].h; arr[i].w = arr_img[i].w
        arr[i].on_device = (OP_SRC_DEVICE if arr_img[i].on_device else 0) | (OP_SRC_U8 if arr_img[i].dtype == OP_U8 else 0)
    return arr, keep


class _View:
    """``__cuda_array_interface__`` over a device buffer of ``owner``, which the view keeps alive"""

    def __init__(self, owner, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr or 0), False), "version": 2, "strides": None}
        self._owner = owner


class Features(_Handle):
    """``op_features``: device-resident descriptors/coordinates of a batch of images."""
    _free_fn = "op_features_free"

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self.handle = handle

    @property
    def num_images(self):
        return lib().op_features_num_images(self.handle)

    def count(self, i):
        return lib().op_features_count(self.handle, i)

    @property
    def total(self):
        return lib().op_features_total(self.handle)

    def offset(self, i):
        return lib().op_features_offset(self.handle, i)

    @property
    def desc_ptr(self):
        return lib().op_features_desc_device(self.handle)

    @property
    def coor_ptr(self):
        return lib().op_features_coor_device(self.handle)

    def get(self, i):
        k = self.count(i)
        desc = np.empty((k, 128), np.float32); coor = np.empty((k, 2), np.float64)
        check(lib().op_features_copy(self.ctx.handle, self.handle, i, _p(desc), _p(coor)))
        return desc, coor

    def get_real(self, i):
        """real_coor in [0,1) of image i (what do_detect_feature itself returns, feature.cc:31-47)"""
        k = self.count(i)
        real = np.empty((k, 2), np.float64)
        check(lib().op_features_copy_real(self.ctx.handle, self.handle, i, _p(real)))
        return real

    @classmethod
    def from_host(cls, ctx, descs, coors=None):
        n = len(descs)
        descs = [np.ascontiguousarray(d, np.float32).reshape(-1, 128) for d in descs]
        dp = (C.c_void_p * n)(*[_p(d) for d in descs])
        if coors is not None:
            coors = [np.ascontiguousarray(c, np.float64).reshape(-1, 2) for c in coors]
            cp = (C.c_void_p * n)(*[_p(c) for c in coors])
        else:
            cp = None
        counts = (C.c_int * n)(*[len(d) for d in descs])
        return cls(ctx, _new(lib().op_features_from_host, ctx.handle, dp, cp, counts, n))

    @classmethod
    def from_device(cls, ctx, desc_ptr, counts, coor_ptr=None):
        """flat device buffer (images back to back, total x 128 fp32) -> Features (D2D copy)"""
        n = len(counts)
        cc = (C.c_int * n)(*[int(c) for c in counts])
        return cls(ctx, _new(lib().op_features_from_device, ctx.handle, C.c_void_p(int(desc_ptr)),
                             C.c_void_p(int(coor_ptr)) if coor_ptr else None, cc, n))

    @classmethod
    def adopt_device(cls, ctx, desc_ptr, counts, coor_ptr, keep=None):
        """flat device buffers (images back to back) -> Features WITHOUT a copy; `keep` (e.g. the torch tensors that own
        the memory) is held until free()"""
        n = len(counts)
        cc = (C.c_int * n)(*[int(c) for c in counts])
        f = cls(ctx, _new(lib().op_features_adopt_device, ctx.handle, C.c_void_p(int(desc_ptr)), C.c_void_p(int(coor_ptr)), cc, n))
        f._keep = keep
        return f

    def desc_device_array(self):
        """object exposing ``__cuda_array_interface__`` over the device descriptor buffer
        (zero-copy view for torch.as_tensor(..., device='cuda'); valid while self is alive)"""
        return _View(self, self.desc_ptr, (int(self.total), 128), "<f4")

    def coor_device_array(self):
        """same for the (total, 2) float64 keypoint coordinates"""
        return _View(self, self.coor_ptr, (int(self.total), 2), "<f8")


def sift_batch(ctx: Context, cfg, images) -> Features:
    arr, keep = _mk_images(images)
    h = _new(lib().op_sift_batch, ctx.handle, _cfg(cfg), arr, len(images))
    del keep
    return Features(ctx, h)


class SiftCall:
    """op_sift_batch with its arguments marshalled once: a host program calling the C-ABI keeps its
    op_image array and op_config around; rebuilding them in Python costs ~35 us per call, which is
    2 % of a 38-image batch on this GPU."""

    def __init__(self, ctx: Context, cfg, images):
        self.ctx = ctx
        self.arr, self.keep = _mk_images(images)
        self.n = len(images)
        self.ccfg = OpConfig.from_config(cfg)
        self._fn = lib().op_sift_batch

    def __call__(self) -> Features:
        h = C.c_void_p()
        check(self._fn(self.ctx.handle, C.byref(self.ccfg), self.arr, self.n, C.byref(h)))
        return Features(self.ctx, h)


class SiftHostCall:
    """op_sift_batch_host with its arguments marshalled once: host images in, descriptors / coordinates into the given
    host buffers (raw pointers, e.g. pinned torch tensors' data_ptr()), transfers overlapped with the kernels."""

    def __init__(self, ctx: Context, cfg, images, desc_ptr, coor_ptr, capacity_rows):
        self.ctx = ctx
        self.arr, self.keep = _mk_images(images)
        self.n = len(images)
        self.ccfg = OpConfig.from_config(cfg)
        self.desc_ptr = C.c_void_p(int(desc_ptr)) if desc_ptr else None
        self.coor_ptr = C.c_void_p(int(coor_ptr)) if coor_ptr else None
        self.cap = int(capacity_rows)

    def __call__(self) -> Features:
        h = C.c_void_p()
        rc = lib().op_sift_batch_host(self.ctx.handle, C.byref(self.ccfg), self.arr, self.n, self.desc_ptr, self.coor_ptr, self.cap, C.byref(h))
        if rc != 0 and h:
            lib().op_features_free(h)           # OP_ERR_CAPACITY still hands over the resident features
        check(rc)
        return Features(self.ctx, h)


def sift_staged(ctx: Context, cfg, image, planes=True):
    """Staged single-image run -> object with the same fields as tests' ``SiftStages``."""
    L = lib()
    arr, keep = _mk_images([image])
    hd = _new(L.op_sift_staged, ctx.handle, _cfg(cfg), arr)

    class Stages:
        pass

    st = Stages()
    try:
        h, w = C.c_int(), C.c_int()
        L.op_sift_dump_working_dims(hd, C.byref(h), C.byref(w))
        st.work = np.empty((h.value, w.value, 3), np.float32)
        check(L.op_sift_dump_plane(ctx.handle, hd, 4, 0, 0, _p(st.work)))
        st.dims = []; st.grey = {}; st.dog = {}; st.mag = {}; st.ort = {}; st.raw = {}
        for o in range(cfg.NUM_OCTAVE):
            check(L.op_sift_dump_octave_dims(hd, o, C.byref(h), C.byref(w)))
            st.dims.append((h.value, w.value))
            if planes:
                def grab(kind, s):
                    buf = np.empty((h.value, w.value), np.float32)
                    check(L.op_sift_dump_plane(ctx.handle, hd, kind, o, s, _p(buf)))
                    return buf
                st.grey[o] = grab(5, 0)
                for s in range(cfg.NUM_SCALE - 1):
                    st.dog[(o, s)] = grab(1, s)
                for s in range(1, cfg.NUM_SCALE - 2):
                    st.mag[(o, s)] = grab(2, s)
                    st.ort[(o, s)] = grab(3, s)
            for s in range(1, cfg.NUM_SCALE - 2):
                n = L.op_sift_dump_raw_count(hd, o, s)
                xy = np.empty((n, 2), np.int32)
                if n:
                    L.op_sift_dump_raw(hd, o, s, _p(xy))
                st.raw[(o, s)] = xy
        for which, name in ((0, "refined"), (1, "oriented")):
            n = L.op_sift_dump_kp_count(hd, which)
            ints = np.empty((n, 4), np.int32); real = np.empty((n, 2), np.float64); fl = np.empty((n, 2), np.float32)
            if n:
                L.op_sift_dump_kp(hd, which, _p(ints), _p(real), _p(fl))
            setattr(st, name, dict(ints=ints, real=real, fl=fl))
        k = L.op_sift_dump_kp_count(hd, 1)
        st.desc = np.empty((k, 128), np.float32); st.coor = np.empty((k, 2), np.float64)
        if k:
            L.op_sift_dump_desc(hd, _p(st.desc), _p(st.coor))
    finally:
        L.op_sift_dump_free(hd)
    del keep
    return st


def debug_math(ctx: Context, which: int, x, y=None):
    x = np.ascontiguousarray(x, np.float32)
    y = np.ascontiguousarray(y, np.float32) if y is not None else x
    out = np.empty_like(x)
    check(lib().op_debug_math(ctx.handle, which, _p(x), _p(y), x.size, _p(out)))
    return out


class Matches(_Handle):
    """``op_matches`` handle (kept for the RANSAC stage)."""
    _free_fn = "op_matches_free"

    def __init__(self, handle, npairs):
        self.handle = handle; self.npairs = npairs

    def get(self, p):
        """(M, 2) int32 <idx in first, idx in second> of pair p."""
        L = lib()
        n = L.op_matches_count(self.handle, p)
        a = np.empty((n, 2), np.int32)
        if n:
            check(L.op_matches_copy(self.handle, p, _p(a)))
        return a

    def lists(self):
        """every pair's (M, 2) int32 list: one library call, one D2H of the resident lists"""
        L = lib()
        offs = np.empty(self.npairs + 1, np.int64)
        check(L.op_matches_copy_all(self.handle, None, _p(offs)))
        flat = np.empty((int(offs[-1]), 2), np.int32)
        if len(flat):
            check(L.op_matches_copy_all(self.handle, _p(flat), None))
        return [flat[offs[p]: offs[p + 1]] for p in range(self.npairs)]

    @property
    def total(self):
        return int(lib().op_matches_total(self.handle))

    @classmethod
    def from_host(cls, lists):
        lists = [np.ascontiguousarray(a, np.int32).reshape(-1, 2) for a in lists]
        n = len(lists)
        ptrs = (C.c_void_p * n)(*[_p(a) for a in lists])
        counts = (C.c_int * n)(*[len(a) for a in lists])
        return cls(_new(lib().op_matches_from_host, ptrs, counts, n), n)

    @classmethod
    def concat(cls, ctx, a, b):
        """a's pairs followed by b's as one handle (op_matches_concat): one op_ransac_pairs call for both"""
        return cls(_new(lib().op_matches_concat, ctx.handle, a.handle, b.handle), a.npairs + b.npairs)


def _match(owner, cfg, feats, pairs) -> Matches:
    """op_match_pairs on a Context, op_match_pairs_multi on a Group"""
    pr = _pairs(pairs)
    fn = lib().op_match_pairs_multi if isinstance(owner, Group) else lib().op_match_pairs
    return Matches(_new(fn, owner.handle, _cfg(cfg), feats.handle, _p(pr), len(pr)), len(pr))


def match_pairs_handle(ctx: Context, cfg, feats: Features, pairs) -> Matches:
    return _match(ctx, cfg, feats, pairs)


def _ransac(owner, cfg, feats, matches, pairs, shapes_wh, seeds, base_seed):
    """op_ransac_pairs on a Context, op_ransac_pairs_multi on a Group -> (result handle, the pair list as passed): the caller
    reads the result and frees it with op_ransac_free"""
    pr, sh, sd = _pairs(pairs), _shapes(shapes_wh), _seeds(seeds)
    fn = lib().op_ransac_pairs_multi if isinstance(owner, Group) else lib().op_ransac_pairs
    return _new(fn, owner.handle, _cfg(cfg), feats.handle, matches.handle, _p(pr), len(pr), _p(sh), _p(sd), int(base_seed)), pr


def ransac_pairs(ctx: Context, cfg, feats: Features, matches: Matches, pairs, shapes_wh, seeds=None, base_seed=0):
    """Batched TransformEstimation::get_transform. shapes_wh: (n_images, 2) of (w, h).
    -> list of dict(ok, confidence, homo (3,3), inliers, best_hyp, best_count) per pair."""
    L = lib()
    h, pr = _ransac(ctx, cfg, feats, matches, pairs, shapes_wh, seeds, base_seed)
    out = []
    try:
        for p in range(len(pr)):
            homo = np.zeros(9, np.float64)
            check(L.op_ransac_homo(h, p, _p(homo)))
            n = L.op_ransac_inlier_count(h, p)
            inl = np.empty(n, np.int32)
            if n:
                check(L.op_ransac_inliers(h, p, _p(inl)))
            bh = C.c_int(); bc = C.c_int()
            check(L.op_ransac_best(h, p, C.byref(bh), C.byref(bc)))
            out.append(dict(ok=bool(L.op_ransac_ok(h, p)), confidence=L.op_ransac_confidence(h, p), homo=homo.reshape(3, 3),
                            inliers=inl, best_hyp=bh.value, best_count=bc.value))
    finally:
        L.op_ransac_free(h)
    return out


def ransac_pairs_summary(ctx: Context, cfg, feats: Features, matches: Matches, pairs, shapes_wh, base_seed=0, seeds=None):
    """op_ransac_pairs without unpacking every pair into Python: -> (accepted pairs, total inliers)."""
    h, _ = _ransac(ctx, cfg, feats, matches, pairs, shapes_wh, seeds, base_seed)
    try:
        ok = C.c_int(); inl = C.c_int64()
        check(lib().op_ransac_summary(h, C.byref(ok), C.byref(inl)))
        return ok.value, inl.value
    finally:
        lib().op_ransac_free(h)


def ransac_pairwise_table(ctx: Context, cfg, feats: Features, matches: Matches, pairs, shapes_wh, base_seed=0, seeds=None, table_pairs=None):
    """op_ransac_pairs + op_pairwise_table: RANSAC of every pair and Stitcher::match_image's bookkeeping (stitcher.cc:79-93)
    without unpacking a pair into Python.  -> (ij (E, 2) int32, conf (E,) float32, homo (E, 9) float64, cnt (E,) int32,
    pts (sum cnt, 4) float64, accepted pairs): the arguments of pano_estimate_cameras; E = 2 x accepted pairs."""
    L = lib()
    h, pr = _ransac(ctx, cfg, feats, matches, pairs, shapes_wh, seeds, base_seed)
    try:
        ne = C.c_int(); npt = C.c_int64()
        check(L.op_pairwise_table_size(h, C.byref(ne), C.byref(npt)))
        E, P = ne.value, npt.value
        ij = np.zeros((max(E, 1), 2), np.int32); conf = np.zeros(max(E, 1), np.float32); homo = np.zeros((max(E, 1), 9), np.float64)
        cnt = np.zeros(max(E, 1), np.int32); pts = np.zeros((max(P, 1), 4), np.float64)
        tp = pr if table_pairs is None else _pairs(table_pairs)   # (tests: a list other than the call's is refused)
        check(L.op_pairwise_table(ctx.handle, feats.handle, matches.handle, h, _p(tp), len(tp), _p(ij), _p(conf), _p(homo), _p(cnt), _p(pts)))
        return ij[:E], conf[:E], homo[:E], cnt[:E], pts[:P], E // 2
    finally:
        L.op_ransac_free(h)


def match_pairs(ctx: Context, cfg, feats: Features, pairs):
    """All requested image pairs in one call -> list of (M, 2) int32 arrays of
    <idx in image i, idx in image j>, sorted by (first, second) (``MatchData``, matcher.hh:14-25)."""
    mh = _match(ctx, cfg, feats, pairs)
    try:
        return [a.copy() for a in mh.lists()]
    finally:
        mh.free()


class Canvas(_Handle):
    """``op_canvas``: device-resident H x W x 3 fp32 result of a blend / warp."""
    _free_fn = "op_canvas_free"

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx; self.handle = handle
        h, w = C.c_int(), C.c_int()
        check(lib().op_canvas_dims(handle, C.byref(h), C.byref(w)))
        self.h, self.w = h.value, w.value

    @property
    def device_ptr(self):
        return lib().op_canvas_device(self.handle)

    def numpy(self):
        out = np.empty((self.h, self.w, 3), np.float32)
        check(lib().op_canvas_copy(self.ctx.handle, self.handle, _p(out)))
        return out

    @classmethod
    def upload(cls, ctx: Context, array) -> "Canvas":
        """a device canvas from an (H, W, 3) float32 host image, Color::NO = -1 allowed (op_canvas_upload)"""
        a = np.ascontiguousarray(array, np.float32)
        if a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"Canvas.upload: expected (H, W, 3) float32, got {a.shape}")
        return cls(ctx, _new(lib().op_canvas_upload, ctx.handle, _p(a), a.shape[0], a.shape[1]))

    def perspective(self, inv, cfg) -> "Canvas":
        """CylinderStitcher::perspective_correction's LinearBlender pass (cylstitcher.cc:170-179) under cfg's ORDERED_INPUT and
        LAZY_READ: pixel (i, j) of the result samples this canvas at trans2d(j, i) of ``inv`` (op_canvas_perspective)"""
        m = np.ascontiguousarray(np.asarray(inv, np.float64).reshape(9))
        return Canvas(self.ctx, _new(lib().op_canvas_perspective, self.ctx.handle, _cfg(cfg), self.handle, _p(m)))

    def reproject(self, frame: OpPanoFrame, spec: OpViewSpec) -> "Canvas":
        """this equirectangular canvas, lying at ``frame`` (pano_frame, or an OpPanoFrame of the caller's), looked at as ``spec``
        says (view_look, view_cube_face, view_planet) -> a new canvas of spec.out_h x spec.out_w, Color::NO where nothing is
        sampled (op_canvas_reproject)"""
        return Canvas(self.ctx, _new(lib().op_canvas_reproject, self.ctx.handle, self.handle, C.byref(frame), C.byref(spec)))

    def crop(self):
        """crop() of the reference (lib/imgproc.cc:200-235) -> (Canvas, (x0, y0))"""
        h = C.c_void_p(); x0, y0 = C.c_int(), C.c_int()
        check(lib().op_canvas_crop(self.ctx.handle, self.handle, C.byref(h), C.byref(x0), C.byref(y0)))
        return Canvas(self.ctx, h), (x0.value, y0.value)

    def numpy_u8(self):
        """write_rgb quantisation on the device, bytes over PCIe"""
        out = np.empty((self.h, self.w, 3), np.uint8)
        check(lib().op_canvas_copy_u8(self.ctx.handle, self.handle, _p(out)))
        return out

    def png_bytes(self) -> bytes:
        """the canvas as a PNG file (8-bit RGB, numpy_u8()'s pixels), encoded on the device (op_canvas_encode_png)"""
        return _take_file(self.ctx, _new(lib().op_canvas_encode_png, self.ctx.handle, self.handle), "op_png")

    def write_png(self, path):
        _write(path, self.png_bytes())

    def jpeg_bytes(self, quality=90, subsampling="420") -> bytes:
        """the canvas as a baseline JPEG file (numpy_u8()'s pixels; every byte what libjpeg writes for them at this quality and
        sampling, with restart markers), encoded on the device (op_canvas_encode_jpeg)"""
        h = _new(lib().op_canvas_encode_jpeg, self.ctx.handle, self.handle, int(quality), _jpeg_subsampling(subsampling))
        return _take_file(self.ctx, h, "op_jpeg")

    def write_jpeg(self, path, quality=90, subsampling="420"):
        _write(path, self.jpeg_bytes(quality, subsampling))


def _take_file(ctx: Context, handle, prefix) -> bytes:
    """the bytes of an encoded-file handle (prefix: "op_png" or "op_jpeg"), which is freed"""
    size, copy, free = (getattr(lib(), f"{prefix}_{f}") for f in ("size", "copy", "free"))
    try:
        out = np.empty(size(handle), np.uint8)
        check(copy(ctx.handle, handle, _p(out)))
        return out.tobytes()
    finally:
        free(handle)


def _rgb_u8(array, who):
    a = np.ascontiguousarray(array, np.uint8)
    if a.ndim != 3 or a.shape[2] != 3:
        raise ValueError(f"{who}: expected (H, W, 3) bytes, got {a.shape}")
    return a


def encode_png_u8(ctx: Context, array) -> bytes:
    """PNG file of an (H, W, 3) uint8 array in host memory, through the device encoder (op_png_encode_u8)"""
    a = _rgb_u8(array, "encode_png_u8")
    return _take_file(ctx, _new(lib().op_png_encode_u8, ctx.handle, _p(a), a.shape[0], a.shape[1]), "op_png")


JPEG_444, JPEG_420 = 0, 1      # OP_JPEG_444, OP_JPEG_420


def _jpeg_subsampling(s) -> int:
    """"444" / "420" or the C enum; anything else goes to the library as it is (an int) and comes back as OP_ERR_INVALID"""
    if isinstance(s, str):
        if s not in ("444", "420"):
            raise ValueError(f"subsampling: '444' or '420', got {s!r}")
        return JPEG_444 if s == "444" else JPEG_420
    return int(s)


def encode_jpeg_u8(ctx: Context, array, quality=90, subsampling="420") -> bytes:
    """JPEG file of an (H, W, 3) uint8 array in host memory, through the device encoder (op_jpeg_encode_u8)"""
    a = _rgb_u8(array, "encode_jpeg_u8")
    h = _new(lib().op_jpeg_encode_u8, ctx.handle, _p(a), a.shape[0], a.shape[1], int(quality), _jpeg_subsampling(subsampling))
    return _take_file(ctx, h, "op_jpeg")


def blend_prepare(cfg, shapes_wh, homos, proj_method, identity_idx):
    """Host geometry of ``ConnectedImages`` (calc_inverse_homo, update_proj_range,
    get_final_resolution: stitcher_image.cc:36-114) -> (OpBlendGeom, homo_inv (n,9), ranges (n,4))."""
    sh = _shapes(shapes_wh)
    n = len(sh)
    homo = np.ascontiguousarray(np.asarray(homos, np.float64).reshape(n, 9))
    g = OpBlendGeom(); hinv = np.zeros((n, 9), np.float64); ranges = np.zeros((n, 4), np.float64)
    check(lib().op_blend_prepare(_cfg(cfg), int(proj_method), int(identity_idx), n, _p(sh), _p(homo), C.byref(g), _p(hinv), _p(ranges)))
    return g, hinv, ranges


GAIN_FIX = 2.0 ** 32                  # fixed-point scale of op_gain_overlap's colour sums
GAIN_SIGMA_N, GAIN_SIGMA_G = 10.0 / 255.0, 0.1
GAIN_SIGMA_S = 0.1                    # smoothness of block gains (op_gain_block_solve)
GAIN_BLOCK_MAX_ENTRIES = 1 << 22      # op_gain_block_overlap's cap on pairs x (bx by)^2 (include/openpano_hip.h)
VIG_SIGMA_N, VIG_SIGMA_G, VIG_SIGMA_V = 10.0 / 255.0, 1.0, 100.0   # op_vignette_solve's usual priors
VIG_STRIDE, VIG_CLIP = 2, 0.98        # op_vignette_overlap's usual lattice stride and saturation clip
VIG_MOMENTS = 30                      # moments per pair: A_0..6, B_0..6, C_00..33


def _gains_array(gains, n):
    """(n, 3) per-image gains, or (n, by, bx, 3) block gains (4-d); (n,) = one gain per image"""
    if gains is None:
        return None
    g = np.ascontiguousarray(np.asarray(gains, np.float32))
    if g.ndim == 4:
        if g.shape[0] != n or g.shape[3] != 3:
            raise ValueError(f"block gains must be ({n}, by, bx, 3), got {g.shape}")
        return g
    if g.size == n:                    # one gain per image: all three channels
        g = np.ascontiguousarray(np.repeat(g.reshape(n, 1), 3, axis=1))
    if g.shape != (n, 3):
        raise ValueError(f"gains must be ({n}, 3) or ({n},), got {g.shape}")
    return g


class BlendCall:
    """``ConnectedImages::blend()`` (stitcher_image.cc:116-155) with the op_blend_geom / op_blend_image arrays marshalled
    once, like a C host holds them; every call is one op_blend -- or, with ``gains`` ((n, 3) or (n,) exposure gains), one
    op_blend_gains; with (n, by, bx, 3) block gains, one op_blend_block_gains; with ``vignette`` (a1, a2, a3: the shared
    curve of op_vignette_solve), one op_blend_vignette of ``gains`` ((n, 3), (n,) or None = 1).
    images: numpy HWC float32 or uint8 (decoder bytes) arrays, (device_ptr, h, w) / (device_ptr, h, w, "u8") tuples, or a
    ``Views``; byte sources are converted in the sampler (OP_SRC_U8).  homos: n x 3 x 3 ImageComponent::homo."""

    def __init__(self, ctx: Context, cfg, images, homos, proj_method, identity_idx, gains=None, vignette=None):
        self.ctx = ctx
        n = self.n = len(images)
        arr, self._keep = _mk_blend_images(images)
        self.arr = arr
        shapes = [(arr[i].w, arr[i].h) for i in range(n)]
        self.geom, hinv, ranges = blend_prepare(cfg, shapes, homos, proj_method, identity_idx)
        for i in range(n):
            for k in range(9):
                arr[i].homo_inv[k] = hinv[i, k]
            for k in range(4):
                arr[i].range[k] = ranges[i, k]
        self.ccfg = OpConfig.from_config(cfg)
        self.gains = _gains_array(gains, n)
        self.vignette = None
        if vignette is not None:
            self.vignette = np.ascontiguousarray(np.asarray(vignette, np.float32).reshape(-1))
            if self.vignette.shape != (3,):
                raise ValueError(f"vignette must hold the 3 coefficients a1, a2, a3, got {self.vignette.shape}")
            if self.gains is not None and self.gains.ndim != 2:
                raise ValueError("vignetting takes per-image gains (n, 3), not block gains")
        self._gains_p, self._vignette_p = _p(self.gains), _p(self.vignette)      # of the arrays this object keeps
        self._fn = lib().op_blend

    def __call__(self) -> Canvas:
        h = C.c_void_p()
        if self.vignette is not None:
            check(lib().op_blend_vignette(self.ctx.handle, C.byref(self.ccfg), C.byref(self.geom), self.arr, self.n,
                                          self._gains_p, self._vignette_p, C.byref(h)))
        elif self.gains is None:
            check(self._fn(self.ctx.handle, C.byref(self.ccfg), C.byref(self.geom), self.arr, self.n, C.byref(h)))
        elif self.gains.ndim == 4:
            by, bx = self.gains.shape[1:3]
            check(lib().op_blend_block_gains(self.ctx.handle, C.byref(self.ccfg), C.byref(self.geom), self.arr, self.n, int(bx), int(by),
                                             self._gains_p, C.byref(h)))
        else:
            check(lib().op_blend_gains(self.ctx.handle, C.byref(self.ccfg), C.byref(self.geom), self.arr, self.n, self._gains_p, C.byref(h)))
        return Canvas(self.ctx, h)

    def _overlap(self, fn, args, per_pair):
        """one of the three overlap passes over this call's canvas -> (count, sums): per pair, sums of shape ``per_pair`` and
        one count for each of their last axes"""
        npairs = self.n * (self.n - 1) // 2
        rows = max(npairs, 1)
        count = np.zeros((rows,) + per_pair[:-1], np.int64); sums = np.zeros((rows,) + per_pair, np.int64)
        check(fn(self.ctx.handle, C.byref(self.ccfg), C.byref(self.geom), self.arr, self.n, *args, _p(count), _p(sums)))
        return count[:npairs], sums[:npairs]

    def overlap_sums(self, stride=1):
        """op_gain_overlap over this call's canvas -> (count (P,) int64, sums (P, 6) int64: S_ab[3], S_ba[3] in units of
        2^-32), P = n (n - 1) / 2, pair (a < b) at index pair_index(n, a, b)."""
        return self._overlap(lib().op_gain_overlap, (int(stride),), (6,))

    def vignette_overlap_sums(self, stride=VIG_STRIDE, clip=VIG_CLIP):
        """op_vignette_overlap over this call's canvas -> (count (P,) int64, moments (P, 30) int64 in units of 2^-32):
        A_k = sum Ya^2 rho_b^k at [p, k], B_k = sum Yb^2 rho_a^k at [p, 7 + k] (k = 0..6), C_ij = sum Ya Yb rho_a^i rho_b^j
        at [p, 14 + 4 i + j] (i, j = 0..3); samples whose largest channel exceeds clip are left out."""
        return self._overlap(lib().op_vignette_overlap, (int(stride), float(clip)), (VIG_MOMENTS,))

    def block_overlap_sums(self, bx, by, stride=1):
        """op_gain_block_overlap -> (count (P, B, B) int64, sums (P, B, B, 6) int64 fixed point), B = bx * by: the entry
        [p, qa, qb] holds the samples of pair p = pair_index(n, a, b) whose a-side lies in block qa = v * bx + u of image a
        and b-side in block qb of image b."""
        npairs, B = self.n * (self.n - 1) // 2, int(bx) * int(by)
        if npairs * B * B > GAIN_BLOCK_MAX_ENTRIES:       # refused by the library; do not allocate the arrays first
            raise OpenPanoHipError(f"op_gain_block_overlap: {npairs * B * B} unit-pair entries exceed {GAIN_BLOCK_MAX_ENTRIES}")
        return self._overlap(lib().op_gain_block_overlap, (int(stride), int(bx), int(by)), (B, B, 6))


def blend(ctx: Context, cfg, images, homos, proj_method, identity_idx, gains=None, vignette=None) -> Canvas:
    """``ConnectedImages::blend()`` (stitcher_image.cc:116-155) on the device.
    images: numpy HWC float32 / uint8 arrays, device tuples (ptr, h, w[, "u8"]) or a ``Views``; homos: n x 3 x 3
    ImageComponent::homo.
    gains: optional (n, 3) or (n,) exposure gains (op_blend_gains), or (n, by, bx, 3) block gains (op_blend_block_gains);
    None = op_blend.  vignette: optional (a1, a2, a3), the shared curve of vignette_solve (op_blend_vignette, with gains)."""
    return BlendCall(ctx, cfg, images, homos, proj_method, identity_idx, gains=gains, vignette=vignette)()


def pair_index(n, a, b):
    """index of the pair (a < b) in op_gain_overlap's arrays"""
    return a * n - a * (a + 1) // 2 + (b - a - 1)


def gain_overlap_sums(ctx: Context, cfg, images, homos, proj_method, identity_idx, stride=1):
    """op_gain_overlap -> (count (P,) int64, sums (P, 6) int64 fixed point, 2^32 = 1.0)"""
    return BlendCall(ctx, cfg, images, homos, proj_method, identity_idx).overlap_sums(stride)


def gain_overlap(ctx: Context, cfg, images, homos, proj_method, identity_idx, stride=1):
    """Overlap statistics of exposure compensation (op_gain_overlap) -> (count (P,) int64, means (P, 6) float64):
    means[p] = (I_ab[3], I_ba[3]), the mean colour of image a and of image b over their common valid samples
    (0 where count is 0); pair (a < b) at pair_index(n, a, b)."""
    count, sums = gain_overlap_sums(ctx, cfg, images, homos, proj_method, identity_idx, stride)
    den = GAIN_FIX * np.maximum(count, 1).astype(np.float64)
    return count, np.where(count[:, None] > 0, sums.astype(np.float64) / den[:, None], 0.0)


def gain_solve(n, count, sums, sigma_n=GAIN_SIGMA_N, sigma_g=GAIN_SIGMA_G, per_channel=True):
    """op_gain_solve (host only): exposure gains (n, 3) float32 from op_gain_overlap's count / fixed-point sums."""
    npairs = n * (n - 1) // 2
    c = np.ascontiguousarray(np.asarray(count, np.int64).reshape(-1))
    s = np.ascontiguousarray(np.asarray(sums, np.int64).reshape(-1, 6))
    if len(c) != npairs or len(s) != npairs:
        raise ValueError(f"{n} images need {npairs} pairs, got {len(c)} counts and {len(s)} sums")
    out = np.zeros((n, 3), np.float32)
    check(lib().op_gain_solve(int(n), _p(c if npairs else None), _p(s if npairs else None), float(sigma_n), float(sigma_g),
                              int(bool(per_channel)), _p(out)))
    return out


def gain_compensate(ctx: Context, cfg, images, homos, proj_method, identity_idx, stride=1, sigma_n=GAIN_SIGMA_N,
                    sigma_g=GAIN_SIGMA_G, per_channel=True):
    """op_gain_overlap + op_gain_solve: the exposure gains (n, 3) to pass to blend(..., gains=)"""
    count, sums = gain_overlap_sums(ctx, cfg, images, homos, proj_method, identity_idx, stride)
    return gain_solve(len(images), count, sums, sigma_n, sigma_g, per_channel)


def gain_block_solve(n, bx, by, count, sums, sigma_n=GAIN_SIGMA_N, sigma_g=GAIN_SIGMA_G, sigma_s=GAIN_SIGMA_S, per_channel=True):
    """op_gain_block_solve (host only): block gains (n, by, bx, 3) float32 from op_gain_block_overlap's count / sums"""
    npairs, B = n * (n - 1) // 2, int(bx) * int(by)
    c = np.ascontiguousarray(np.asarray(count, np.int64).reshape(-1))
    s = np.ascontiguousarray(np.asarray(sums, np.int64).reshape(-1))
    if len(c) != npairs * B * B or len(s) != 6 * npairs * B * B:
        raise ValueError(f"{n} images at {bx} x {by} need {npairs * B * B} entries, got {len(c)} counts and {len(s) // 6} sums")
    out = np.zeros((n, int(by), int(bx), 3), np.float32)
    check(lib().op_gain_block_solve(int(n), int(bx), int(by), _p(c if npairs else None), _p(s if npairs else None), float(sigma_n),
                                    float(sigma_g), float(sigma_s), int(bool(per_channel)), _p(out)))
    return out


def gain_block_compensate(ctx: Context, cfg, images, homos, proj_method, identity_idx, bx, by, stride=1, sigma_n=GAIN_SIGMA_N,
                          sigma_g=GAIN_SIGMA_G, sigma_s=GAIN_SIGMA_S, per_channel=True):
    """op_gain_block_overlap + op_gain_block_solve: the block gains (n, by, bx, 3) to pass to blend(..., gains=)"""
    call = BlendCall(ctx, cfg, images, homos, proj_method, identity_idx)
    count, sums = call.block_overlap_sums(bx, by, stride)
    return gain_block_solve(len(images), bx, by, count, sums, sigma_n, sigma_g, sigma_s, per_channel)


def vignette_solve(n, count, moments, degree=3, sigma_n=VIG_SIGMA_N, sigma_g=VIG_SIGMA_G, sigma_v=VIG_SIGMA_V):
    """op_vignette_solve (host only): (gains (n, 3) float32, poly (3,) float32 = a1, a2, a3) from op_vignette_overlap's
    count / moments.  Raises OpenPanoHipError (code OP_ERR_UNSUPPORTED) when the fitted curve is not positive on [0, 1]:
    fall back to gain_solve then."""
    npairs = n * (n - 1) // 2
    c = np.ascontiguousarray(np.asarray(count, np.int64).reshape(-1))
    m = np.ascontiguousarray(np.asarray(moments, np.int64).reshape(-1, VIG_MOMENTS))
    if len(c) != npairs or len(m) != npairs:
        raise ValueError(f"{n} images need {npairs} pairs, got {len(c)} counts and {len(m)} moment rows")
    gains = np.zeros((n, 3), np.float32); poly = np.zeros(3, np.float32)
    check(lib().op_vignette_solve(int(n), _p(c if npairs else None), _p(m if npairs else None), int(degree), float(sigma_n),
                                  float(sigma_g), float(sigma_v), _p(gains), _p(poly)))
    return gains, poly


def vignette_compensate(ctx: Context, cfg, images, homos, proj_method, identity_idx, stride=VIG_STRIDE, clip=VIG_CLIP, degree=3,
                        sigma_n=VIG_SIGMA_N, sigma_g=VIG_SIGMA_G, sigma_v=VIG_SIGMA_V):
    """op_vignette_overlap + op_vignette_solve: (gains (n, 3), poly (3,)) to pass to blend(..., gains=gains, vignette=poly)"""
    call = BlendCall(ctx, cfg, images, homos, proj_method, identity_idx)
    count, moments = call.vignette_overlap_sums(stride, clip)
    return vignette_solve(len(images), count, moments, degree, sigma_n, sigma_g, sigma_v)


def pano_frame(geom: OpBlendGeom, x0=0, y0=0, wrap=False) -> OpPanoFrame:
    """the frame of the canvas a spherical blend made from ``geom`` (BlendCall.geom), or of its crop at (x0, y0)
    (op_pano_frame_of, host only).  wrap is the caller's statement that the columns span exactly one turn: never guessed."""
    f = OpPanoFrame()
    check(lib().op_pano_frame_of(C.byref(geom), int(x0), int(y0), C.byref(f)))
    f.wrap = int(bool(wrap))
    return f


def view_look(yaw, pitch, roll, hfov, out_w, out_h) -> OpViewSpec:
    """a pinhole view: angles in radians, positive yaw looks right, positive pitch looks up; hfov in (0, pi) (op_view_look)"""
    s = OpViewSpec()
    check(lib().op_view_look(float(yaw), float(pitch), float(roll), float(hfov), int(out_w), int(out_h), C.byref(s)))
    return s


def view_cube_face(face, n) -> OpViewSpec:
    """cube face 0..5 = +x, -x, +y, -y, +z, -z as an n x n view (op_view_cube_face)"""
    s = OpViewSpec()
    check(lib().op_view_cube_face(int(face), int(n), C.byref(s)))
    return s


def view_planet(n) -> OpViewSpec:
    """the reference's "little planet" of n x n pixels (op_view_planet)"""
    s = OpViewSpec()
    check(lib().op_view_planet(int(n), C.byref(s)))
    return s


def perspective_homography(proj_min, ref_wh, first_wh, first_homo, last_wh, last_homo, canvas_wh):
    """Host geometry of ``CylinderStitcher::perspective_correction`` (cylstitcher.cc:140-168) -> (inv (3, 3), corners (4, 2)).
    proj_min: the bundle's ``proj_range.min`` (an OpBlendGeom or an (x, y) pair); *_wh: (w, h) of the reference view, of the first
    and the last component's ImageRef and of the canvas; *_homo: the first and the last ``component.homo``."""
    if isinstance(proj_min, OpBlendGeom):
        g = proj_min
    else:
        g = OpBlendGeom()
        g.proj_min[0], g.proj_min[1] = float(proj_min[0]), float(proj_min[1])
    fh = np.ascontiguousarray(np.asarray(first_homo, np.float64).reshape(9))
    lh = np.ascontiguousarray(np.asarray(last_homo, np.float64).reshape(9))
    inv = np.zeros(9); corners = np.zeros(8)
    check(lib().op_perspective_homography(C.byref(g), int(ref_wh[0]), int(ref_wh[1]), int(first_wh[0]), int(first_wh[1]), _p(fh),
                                          int(last_wh[0]), int(last_wh[1]), _p(lh), int(canvas_wh[0]), int(canvas_wh[1]),
                                          _p(inv), _p(corners)))
    return inv.reshape(3, 3), corners.reshape(4, 2)


def cyl_warp_shape(cfg, w, h, h_factor, pts=None):
    """Host part of ``CylinderWarper::warp`` -> (new_w, new_h, offset (2,), warped centred pts)."""
    p = np.ascontiguousarray(pts, np.float64).reshape(-1, 2).copy() if pts is not None else np.zeros((0, 2))
    nw, nh = C.c_int(), C.c_int(); off = np.zeros(2)
    check(lib().op_cyl_warp_shape(_cfg(cfg), int(w), int(h), float(h_factor), _p(p if len(p) else None), len(p),
                                  C.byref(nw), C.byref(nh), _p(off)))
    return nw.value, nh.value, off, p


def cyl_warp(ctx: Context, cfg, image, h_factor) -> Canvas:
    """``CylinderWarper::warp``'s pixels; image: float32, or uint8 decoder bytes (host array or device tuple)"""
    arr, keep = _mk_images([image])
    h = _new(lib().op_cyl_warp, ctx.handle, _cfg(cfg), arr, float(h_factor))
    del keep
    return Canvas(ctx, h)
