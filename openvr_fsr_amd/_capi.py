"""ctypes declarations for include/openvr_fsr_amd.h (kept in the same order as the header)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

FORMAT_RGBA8, FORMAT_RGBA16F, FORMAT_RGBA32F, FORMAT_RGB10A2, FORMAT_BGRA8 = 0, 1, 2, 3, 4
FORMAT_R11G11B10F = 6  # OVRFSR_FORMAT_R11G11B10F: input-only packed float (5 is unassigned and refused: header)
FORMAT_SAMPLES_SHIFT = 8  # OVRFSR_FORMAT_SAMPLES_SHIFT: multisampled inputs carry the sample count in the format's high bits


def format_ms(fmt, samples):
    """OVRFSR_FORMAT_MS(fmt, samples): the format value of a multisampled input image (samples 2, 4 or 8; 0 / 1 = single-sample)."""
    return int(fmt) | int(samples) << FORMAT_SAMPLES_SHIFT


PRECISION_FP32, PRECISION_FP32_STRICT = 0, 2
PRECISION_FP32_EXACT = 3  # FP32's arithmetic; every UNORM8 byte stored is the strict build's (header, ovrfsr_precision)
EYE_LEFT, EYE_RIGHT = 0, 1
HDR_DOMAIN_LINEAR, HDR_DOMAIN_SRTM = 0, 1  # ovrfsr_set_hdr_domain: float submissions filtered as submitted / in FSR 1's reversible tone-mapped domain

STATUS = {0: "OK", 1: "INVALID_ARGUMENT", 2: "UNSUPPORTED", 3: "HIP", 4: "NO_DEVICE", 5: "DISABLED", 6: "OUT_OF_MEMORY"}


class OvrFsrError(RuntimeError):
    def __init__(self, status, msg=""):
        super().__init__("ovrfsr status %s (%d): %s" % (STATUS.get(status, "?"), status, msg))
        self.status = status


class Image(C.Structure):
    """ovrfsr_image"""
    _fields_ = [("data", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32),
                ("pitch_bytes", C.c_uint32), ("format", C.c_uint32)]


class Bounds(C.Structure):
    """ovrfsr_bounds == vr::VRTextureBounds_t"""
    _fields_ = [("uMin", C.c_float), ("vMin", C.c_float), ("uMax", C.c_float), ("vMax", C.c_float)]


class Config(C.Structure):
    """ovrfsr_config: the numeric part of the reference's Config singleton (Config.h:10-17)."""
    _fields_ = [("struct_size", C.c_uint32), ("fsr_enabled", C.c_int32), ("use_nis", C.c_int32),
                ("debug_mode", C.c_int32), ("render_scale", C.c_float), ("sharpness", C.c_float),
                ("radius", C.c_float), ("proj_centre", C.c_float * 4), ("out_width", C.c_uint32),
                ("out_height", C.c_uint32), ("precision", C.c_int32), ("quantize_intermediate", C.c_int32),
                ("fused", C.c_int32), ("stage_mask", C.c_int32), ("pair_submit", C.c_int32), ("reference_formats", C.c_int32),
                ("reserved", C.c_int32 * 1)]

    @classmethod
    def default(cls, **kw):
        cfg = cls()
        library().ovrfsr_config_default(C.byref(cfg))
        for k, v in kw.items():
            if k == "proj_centre":
                for i in range(4):
                    cfg.proj_centre[i] = v[i]
            else:
                if not hasattr(cfg, k):
                    raise AttributeError(k)
                setattr(cfg, k, v)
        return cfg


def library_path():
    # OVRFSR_LIB: A/B benchmarking of two builds of the same library in one gpurun call (tools/ab.sh)
    return os.environ.get("OVRFSR_LIB") or os.path.join(_HERE, "libopenvr_fsr_amd.so")


def have_library():
    return os.path.exists(library_path())


def library():
    """Load libopenvr_fsr_amd.so.  Raises if it has not been built: there is no fallback."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = library_path()
    if not os.path.exists(path):
        raise OvrFsrError(4, "%s not built -- run `python -c 'import __graft_entry__ as g; g.build()'`" % path)
    L = C.CDLL(path)
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)
    L.ovrfsr_abi_version.restype = C.c_uint32
    L.ovrfsr_config_default.argtypes = [C.POINTER(Config)]
    L.ovrfsr_config_default.restype = None
    L.ovrfsr_create.argtypes = [C.c_int, C.POINTER(Config), C.POINTER(C.c_void_p)]
    L.ovrfsr_destroy.argtypes = [C.c_void_p]
    L.ovrfsr_destroy.restype = None
    L.ovrfsr_set_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    L.ovrfsr_get_config.argtypes = [C.c_void_p, C.POINTER(Config)]
    L.ovrfsr_reset.argtypes = [C.c_void_p]
    L.ovrfsr_output_size.argtypes = [C.POINTER(Config), C.c_uint32, C.c_uint32, u32p, u32p]
    L.ovrfsr_apply.argtypes = [C.c_void_p, C.c_int, C.POINTER(Image), C.POINTER(Bounds), C.POINTER(Image), C.c_void_p]
    L.ovrfsr_apply_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.POINTER(Image), C.c_size_t,
                                     C.POINTER(Image), C.c_size_t, C.c_void_p]
    L.ovrfsr_apply_batch_shared.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(Image), C.c_size_t, C.POINTER(Image), C.c_size_t, C.c_void_p]
    L.ovrfsr_last_error.argtypes = [C.c_void_p]
    L.ovrfsr_last_error.restype = C.c_char_p
    L.ovrfsr_last_gpu_time_ms.argtypes = [C.c_void_p, f32p]
    L.ovrfsr_average_gpu_time_ms.argtypes = [C.c_void_p, f32p, u32p]
    L.ovrfsr_easu_con.argtypes = [u32p] + [C.c_float] * 6
    L.ovrfsr_easu_con.restype = None
    L.ovrfsr_rcas_con.argtypes = [u32p, C.c_float]
    L.ovrfsr_rcas_con.restype = None
    L.ovrfsr_mask_constants.argtypes = [u32p, u32p, C.c_uint32, C.c_uint32, f32p, C.c_float, C.c_int, C.c_int]
    L.ovrfsr_mask_constants.restype = None
    L.ovrfsr_nis_scaler_config.argtypes = [C.c_void_p, C.c_float] + [C.c_uint32] * 4
    L.ovrfsr_nis_sharpen_config.argtypes = [C.c_void_p, C.c_float] + [C.c_uint32] * 2
    L.ovrfsr_nis_coef_scale.restype = f32p
    L.ovrfsr_nis_coef_usm.restype = f32p
    L.ovrfsr_config_from_json.argtypes = [C.c_char_p, C.c_size_t, C.POINTER(Config)]
    L.ovrfsr_save_ppm.argtypes = [C.POINTER(Image), C.c_char_p, C.c_void_p]
    L.ovrfsr_save_dds.argtypes = [C.POINTER(Image), C.c_char_p, C.c_void_p]
    L.ovrfsr_pair_pending.argtypes = [C.c_void_p]
    if hasattr(L, "ovrfsr_set_hidden_area"):  # probed by symbol, as a host does: an older build of ABI 5 under OVRFSR_LIB (A/B runs) has none
        L.ovrfsr_set_hidden_area.argtypes = [C.c_void_p, C.c_int, f32p, C.c_uint32]
        L.ovrfsr_hidden_area_stats.argtypes = [C.c_void_p, C.c_int, u32p, u32p]
        L.ovrfsr_hidden_tiles.argtypes = [f32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint8), C.c_size_t]
    if hasattr(L, "ovrfsr_set_hdr_domain"):  # (probed the same way)
        L.ovrfsr_set_hdr_domain.argtypes = [C.c_void_p, C.c_int]
        L.ovrfsr_get_hdr_domain.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.ovrfsr_hdr_map.argtypes = [f32p, f32p, C.c_size_t, C.c_int]
    if hasattr(L, "ovrfsr_set_gaze"):  # (probed the same way)
        L.ovrfsr_set_gaze.argtypes = [C.c_void_p, C.c_int, C.c_float, C.c_float]
        L.ovrfsr_clear_gaze.argtypes = [C.c_void_p, C.c_int]
        L.ovrfsr_get_gaze.argtypes = [C.c_void_p, C.c_int, f32p, C.POINTER(C.c_int)]
        L.ovrfsr_gaze_stats.argtypes = [C.c_void_p, u32p, u32p]
    if hasattr(L, "ovrfsr_set_max_input_size"):  # (probed the same way)
        L.ovrfsr_set_max_input_size.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.ovrfsr_get_max_input_size.argtypes = [C.c_void_p, u32p, u32p]
        L.ovrfsr_rescale_stats.argtypes = [C.c_void_p, u32p, u32p]
    if hasattr(L, "ovrfsr_set_mask_feather"):  # (probed the same way)
        L.ovrfsr_set_mask_feather.argtypes = [C.c_void_p, C.c_float]
        L.ovrfsr_get_mask_feather.argtypes = [C.c_void_p, f32p]
        L.ovrfsr_mask_feather_stats.argtypes = [C.c_void_p, u32p]
        L.ovrfsr_mask_feather_weights.argtypes = [u32p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16), C.POINTER(C.c_uint8), C.c_size_t]
    if L.ovrfsr_abi_version() != 5:
        raise OvrFsrError(1, "ABI version mismatch")
    _LIB = L
    return L


# ---- constants-only helpers (no GPU) -----------------------------------------------------------
def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def easu_con(inW, inH, outW, outH):
    con = np.zeros(16, np.uint32)
    library().ovrfsr_easu_con(_u32p(con), inW, inH, inW, inH, outW, outH)
    return con


def rcas_con(stops):
    con = np.zeros(4, np.uint32)
    library().ovrfsr_rcas_con(_u32p(con), stops)
    return con


def mask_constants(outW, outH, proj, radius, only_one_eye, eye):
    centre, rad = np.zeros(4, np.uint32), np.zeros(4, np.uint32)
    p = np.asarray(proj, np.float32)
    library().ovrfsr_mask_constants(_u32p(centre), _u32p(rad), outW, outH, p.ctypes.data_as(C.POINTER(C.c_float)),
                                    radius, int(only_one_eye), int(eye))
    return centre, rad


def mask_feather_weights(centre, radius_px, feather_px, outW, outH):
    """ovrfsr_mask_feather_weights: ([outH, outW] uint16 w8, [outH, outW] uint8 group-inside flags) of the feather rule (no GPU)."""
    c = np.ascontiguousarray(np.asarray(centre, np.uint32).reshape(4))
    w8, inside = np.zeros((outH, outW), np.uint16), np.zeros((outH, outW), np.uint8)
    rc = library().ovrfsr_mask_feather_weights(_u32p(c), int(radius_px), int(feather_px), int(outW), int(outH),
                                               w8.ctypes.data_as(C.POINTER(C.c_uint16)), inside.ctypes.data_as(C.POINTER(C.c_uint8)), w8.size)
    if rc != 0:
        raise OvrFsrError(rc, "ovrfsr_mask_feather_weights")
    return w8, inside


def nis_scaler_config(sharpness, inW, inH, outW, outH):
    buf = np.zeros(64, np.uint32)
    ok = library().ovrfsr_nis_scaler_config(buf.ctypes.data, sharpness, inW, inH, outW, outH)
    return bool(ok), buf


def nis_sharpen_config(sharpness, inW, inH):
    buf = np.zeros(64, np.uint32)
    ok = library().ovrfsr_nis_sharpen_config(buf.ctypes.data, sharpness, inW, inH)
    return bool(ok), buf


def nis_coefs():
    L = library()
    s = np.ctypeslib.as_array(L.ovrfsr_nis_coef_scale(), shape=(64, 8)).copy()
    u = np.ctypeslib.as_array(L.ovrfsr_nis_coef_usm(), shape=(64, 8)).copy()
    return s, u


def mesh_array(uv):
    """triangles as ovrfsr_set_hidden_area takes them: anything that reshapes to [n, 3, 2] (u, v) -> (contiguous float32 array, n)"""
    m = np.ascontiguousarray(np.asarray(uv if uv is not None else [], np.float32).reshape(-1, 3, 2))
    return m, m.shape[0]


def hidden_tiles(uv, outW, outH, tileW=32, tileH=32):
    """ovrfsr_hidden_tiles: the [tilesY, tilesX] uint8 map of the tiles one eye's mesh hides entirely (no GPU)."""
    m, n = mesh_array(uv)
    tx, ty = (outW + tileW - 1) // tileW, (outH + tileH - 1) // tileH
    hidden = np.zeros((ty, tx), np.uint8)
    rc = library().ovrfsr_hidden_tiles(m.ctypes.data_as(C.POINTER(C.c_float)) if n else None, n, outW, outH, tileW, tileH,
                                       hidden.ctypes.data_as(C.POINTER(C.c_uint8)), hidden.size)
    if rc != 0:
        raise OvrFsrError(rc)
    return hidden


def hdr_map(rgb, inverse=False):
    """ovrfsr_hdr_map: the SRTM mapping (forward, or back with ``inverse``) on an array of RGB triples [..., 3]; float32, same shape (no GPU)."""
    a = np.ascontiguousarray(rgb, np.float32)
    if a.shape[-1:] != (3,):
        raise ValueError("expected RGB triples [..., 3]")
    out = np.empty_like(a)
    rc = library().ovrfsr_hdr_map(a.ctypes.data_as(C.POINTER(C.c_float)), out.ctypes.data_as(C.POINTER(C.c_float)), a.size // 3, int(bool(inverse)))
    if rc != 0:
        raise OvrFsrError(rc)
    return out


def config_from_json(text):
    """Config::Load on the text of an openvr_mod.cfg; returns (status, Config)."""
    cfg = Config()
    b = text.encode() if isinstance(text, str) else text
    rc = library().ovrfsr_config_from_json(b, len(b), C.byref(cfg))
    return rc, cfg


def output_size(cfg, inW, inH):
    w, h = C.c_uint32(), C.c_uint32()
    rc = library().ovrfsr_output_size(C.byref(cfg), inW, inH, C.byref(w), C.byref(h))
    if rc != 0:
        raise OvrFsrError(rc)
    return w.value, h.value
