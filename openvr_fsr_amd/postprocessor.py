"""Python mirror of the reference's vr::PostProcessor surface (src/postprocess/PostProcessor.h:12-13)
over the C ABI: ``apply(eye, texture, bounds)`` / ``reset()``.  torch is used only for device memory
and streams; every pixel is produced by the HIP kernels in libopenvr_fsr_amd.so."""
import ctypes as C

import torch

from . import _capi as K

_TORCH_FMT = {torch.uint8: (K.FORMAT_RGBA8, 4), torch.float16: (K.FORMAT_RGBA16F, 8), torch.float32: (K.FORMAT_RGBA32F, 16)}
_FMT_TORCH = {K.FORMAT_RGBA8: torch.uint8, K.FORMAT_RGBA16F: torch.float16, K.FORMAT_RGBA32F: torch.float32}


def image_of(t, fmt=None):
    """[H, W, 4] device tensor -> ovrfsr_image (no copy); ``fmt`` overrides the format implied by the dtype (e.g.
    K.FORMAT_BGRA8 for a uint8 tensor whose channel order is B,G,R,A).  A [H, W] int32 tensor is an R10G10B10A2_UNORM image (one packed
    dword per texel: R bits 0-9, G 10-19, B 20-29, A 30-31); with ``fmt`` = K.FORMAT_R11G11B10F it is an R11G11B10_FLOAT image (input-only:
    R bits 0-10, G 11-21, B 22-31).  A [H, W, S, 4] tensor (or [H, W, S] int32) is a multisampled input with S
    samples per texel, interleaved (K.format_ms); ``fmt`` then names its base format."""
    if ((t.dim() == 4 and t.shape[3] == 4) or (t.dim() == 3 and t.dtype == torch.int32)) and t.shape[2] in (2, 4, 8):
        if not t.is_cuda:
            raise ValueError("expected a tensor on the GPU")
        samples = t.shape[2]
        flat = t.reshape(t.shape[0], t.shape[1] * samples, *t.shape[3:])  # a view: samples are contiguous within a row
        if flat.data_ptr() != t.data_ptr() or (t.dim() == 4 and (t.stride(2) != 4 or t.stride(3) != 1)) or (t.dim() == 3 and t.stride(2) != 1):
            raise ValueError("samples of a texel must be contiguous")
        img = image_of(flat, fmt)
        img.width = t.shape[1]
        img.format = K.format_ms(img.format, samples)
        return img
    if t.dim() == 2 and t.dtype == torch.int32 and t.is_cuda:
        if t.stride(1) != 1:
            raise ValueError("texels must be contiguous")
        if fmt not in (None, K.FORMAT_RGB10A2, K.FORMAT_R11G11B10F):
            raise ValueError("a packed int32 tensor is an RGB10A2 or an R11G11B10F image")
        return K.Image(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * 4, K.FORMAT_RGB10A2 if fmt is None else fmt)
    if t.dim() != 3 or t.shape[2] != 4 or not t.is_cuda:
        raise ValueError("expected a [H, W, 4] tensor on the GPU")
    if t.stride(2) != 1 or t.stride(1) != 4:
        raise ValueError("texels must be contiguous RGBA")
    dfmt, tb = _TORCH_FMT[t.dtype]
    return K.Image(t.data_ptr(), t.shape[1], t.shape[0], t.stride(0) * t.element_size(), dfmt if fmt is None else fmt)


class PostProcessor:
    def __init__(self, cfg=None, device=None, **cfg_kw):
        self._lib = K.library()
        self._ctx = C.c_void_p()
        if not torch.cuda.is_available():
            raise K.OvrFsrError(4, "no HIP device visible to torch")
        self.device = torch.cuda.current_device() if device is None else int(device)
        self.cfg = cfg if cfg is not None else K.Config.default(**cfg_kw)
        rc = self._lib.ovrfsr_create(self.device, C.byref(self.cfg), C.byref(self._ctx))
        if rc != 0:
            raise K.OvrFsrError(rc, "ovrfsr_create")

    def close(self):
        if self._ctx:
            self._lib.ovrfsr_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != 0:
            raise K.OvrFsrError(rc, (self._lib.ovrfsr_last_error(self._ctx) or b"").decode())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_config(self, cfg):
        self.cfg = cfg
        self._check(self._lib.ovrfsr_set_config(self._ctx, C.byref(cfg)))

    def reset(self):
        """PostProcessor::Reset()"""
        self._check(self._lib.ovrfsr_reset(self._ctx))

    def output_size(self, inW, inH):
        return K.output_size(self.cfg, inW, inH)

    def apply(self, eye, tex, bounds=None, out=None, out_dtype=None, in_format=None):
        """PostProcessor::Apply(eye, texture, bounds).  Returns the tensor the compositor should receive.
        With ``out=None`` and ``out_dtype=None`` the ctx-owned output is wrapped (valid until the next apply)."""
        img = image_of(tex, in_format)
        if out is None and out_dtype is not None:
            ow, oh = self.output_size(tex.shape[1], tex.shape[0])
            shape = (oh, ow) if out_dtype == torch.int32 else (oh, ow, 4)  # int32 = packed R10G10B10A2
            out = torch.empty(shape, dtype=out_dtype, device=tex.device)
        oimg = image_of(out) if out is not None else K.Image()
        b = C.byref(bounds) if bounds is not None else None
        self._check(self._lib.ovrfsr_apply(self._ctx, int(eye), C.byref(img), b, C.byref(oimg), self._stream()))
        if out is not None and oimg.data == out.data_ptr():
            return out
        if oimg.data == tex.data_ptr():
            return tex  # pass-through (fsr disabled)
        return _wrap(oimg, tex.device)

    def apply_batch(self, texs, outs, first_eye=K.EYE_LEFT, alternate_eyes=True, in_format=None, shared=False):
        """texs: [N, H, W, 4], outs: [N, outH, outW, 4] (image i = eye first_eye ^ (i & alternate)); shared=True: every image is a
        side-by-side texture holding both eyes (ovrfsr_apply_batch_shared)."""
        n = texs.shape[0]
        if outs.shape[0] != n:
            raise ValueError("outs holds %d images for a batch of %d" % (outs.shape[0], n))
        i0, o0 = image_of(texs[0], in_format), image_of(outs[0])
        if shared:
            self._check(self._lib.ovrfsr_apply_batch_shared(self._ctx, n, C.byref(i0), texs.stride(0) * texs.element_size(), C.byref(o0),
                                                            outs.stride(0) * outs.element_size(), self._stream()))
            return outs
        self._check(self._lib.ovrfsr_apply_batch(self._ctx, n, int(first_eye), int(bool(alternate_eyes)), C.byref(i0),
                                                 texs.stride(0) * texs.element_size(), C.byref(o0),
                                                 outs.stride(0) * outs.element_size(), self._stream()))
        return outs

    def pair_pending(self):
        """cfg.pair_submit: did the last apply only record its submission (ovrfsr_pair_pending)?"""
        return bool(self._lib.ovrfsr_pair_pending(self._ctx))

    def set_hidden_area(self, eye, uv):
        """ovrfsr_set_hidden_area: one eye's hidden-area mesh, anything that reshapes to [n, 3, 2] (u, v in [0,1] of that eye's image, v = 0 the
        first stored row); None or an empty mesh clears it.  The next apply rebuilds."""
        m, n = K.mesh_array(uv)
        self._check(self._lib.ovrfsr_set_hidden_area(self._ctx, int(eye), m.ctypes.data_as(C.POINTER(C.c_float)) if n else None, n))

    def hidden_area_stats(self, eye):
        """ovrfsr_hidden_area_stats, after an apply: (tiles per image of that eye's list, tiles of them the current plan skips)."""
        total, skipped = C.c_uint32(), C.c_uint32()
        self._check(self._lib.ovrfsr_hidden_area_stats(self._ctx, int(eye), C.byref(total), C.byref(skipped)))
        return total.value, skipped.value

    def set_hdr_domain(self, domain):
        """ovrfsr_set_hdr_domain: K.HDR_DOMAIN_LINEAR (default) or K.HDR_DOMAIN_SRTM -- float submissions are tone-mapped in front of the
        filters and un-mapped behind them.  The next apply rebuilds."""
        self._check(self._lib.ovrfsr_set_hdr_domain(self._ctx, int(domain)))

    def hdr_domain(self):
        """ovrfsr_get_hdr_domain"""
        d = C.c_int()
        self._check(self._lib.ovrfsr_get_hdr_domain(self._ctx, C.byref(d)))
        return d.value

    def set_gaze(self, eye, x, y):
        """ovrfsr_set_gaze: the centre of one eye's sharp disc, in proj_centre's convention ([0,1] of that eye's image, y = 0 the first stored
        row; accepted in [-1, 2]).  Stored only: the next apply that launches the eye re-aims the mask, in place where it can."""
        self._check_arg(self._lib.ovrfsr_set_gaze(self._ctx, int(eye), float(x), float(y)), "ovrfsr_set_gaze")

    def clear_gaze(self, eye):
        """ovrfsr_clear_gaze: the eye's mask centre is cfg.proj_centre's again."""
        self._check_arg(self._lib.ovrfsr_clear_gaze(self._ctx, int(eye)), "ovrfsr_clear_gaze")

    def gaze(self, eye):
        """ovrfsr_get_gaze: ((x, y), is_set) -- the eye's cfg.proj_centre where no gaze is set."""
        xy, is_set = (C.c_float * 2)(), C.c_int()
        self._check_arg(self._lib.ovrfsr_get_gaze(self._ctx, int(eye), xy, C.byref(is_set)), "ovrfsr_get_gaze")
        return (xy[0], xy[1]), bool(is_set.value)

    def gaze_stats(self):
        """ovrfsr_gaze_stats: (re-aims in place, rebuilds) applies performed because of a gaze."""
        reaims, rebuilds = C.c_uint32(), C.c_uint32()
        self._check_arg(self._lib.ovrfsr_gaze_stats(self._ctx, C.byref(reaims), C.byref(rebuilds)), "ovrfsr_gaze_stats")
        return reaims.value, rebuilds.value

    def set_max_input_size(self, max_width, max_height):
        """ovrfsr_set_max_input_size: the largest input the ctx will see (the eye texture's allocation); (0, 0) clears it.  With one set, an
        apply whose input size differs from the planned one re-scales in place where only the input size moved."""
        self._check_arg(self._lib.ovrfsr_set_max_input_size(self._ctx, int(max_width), int(max_height)), "ovrfsr_set_max_input_size")

    def max_input_size(self):
        """ovrfsr_get_max_input_size: (max_width, max_height), (0, 0) where none is set."""
        w, h = C.c_uint32(), C.c_uint32()
        self._check_arg(self._lib.ovrfsr_get_max_input_size(self._ctx, C.byref(w), C.byref(h)), "ovrfsr_get_max_input_size")
        return w.value, h.value

    def rescale_stats(self):
        """ovrfsr_rescale_stats: (re-scales in place, rebuilds) applies performed because of an input-size change while a maximum was set."""
        rescales, rebuilds = C.c_uint32(), C.c_uint32()
        self._check_arg(self._lib.ovrfsr_rescale_stats(self._ctx, C.byref(rescales), C.byref(rebuilds)), "ovrfsr_rescale_stats")
        return rescales.value, rebuilds.value

    def set_mask_feather(self, width):
        """ovrfsr_set_mask_feather: the width of the ramp at the radius mask's edge, in cfg.radius's unit; 0 (the default) is off.  Stored
        only: the apply that launches reads it."""
        self._check_arg(self._lib.ovrfsr_set_mask_feather(self._ctx, float(width)), "ovrfsr_set_mask_feather")

    def mask_feather(self):
        """ovrfsr_get_mask_feather"""
        w = C.c_float()
        self._check_arg(self._lib.ovrfsr_get_mask_feather(self._ctx, C.byref(w)), "ovrfsr_get_mask_feather")
        return w.value

    def mask_feather_stats(self):
        """ovrfsr_mask_feather_stats: launches of the feather pass since the ctx was created."""
        n = C.c_uint32()
        self._check_arg(self._lib.ovrfsr_mask_feather_stats(self._ctx, C.byref(n)), "ovrfsr_mask_feather_stats")
        return n.value

    def _check_arg(self, rc, what):
        if rc != 0:  # (an argument check of the C ABI: it leaves ovrfsr_last_error alone)
            raise K.OvrFsrError(rc, what)

    def last_gpu_time_ms(self):
        ms = C.c_float()
        self._check(self._lib.ovrfsr_last_gpu_time_ms(self._ctx, C.byref(ms)))
        return ms.value


    def average_gpu_time_ms(self):
        """(last published mean of 500 readings in ms -- per frame when each eye has its own texture --, number published):
        the reference's "Average GPU processing time for upscale" log line (PostProcessor.cpp:605-626)."""
        ms, n = C.c_float(), C.c_uint32()
        self._check(self._lib.ovrfsr_average_gpu_time_ms(self._ctx, C.byref(ms), C.byref(n)))
        return ms.value, n.value


def _wrap(img, device):
    """View ctx-owned device memory as a torch tensor without copying (via __cuda_array_interface__)."""

    class _Holder:
        pass

    h = _Holder()
    if img.format == K.FORMAT_RGB10A2:   # one packed dword per texel
        h.__cuda_array_interface__ = {"shape": (img.height, img.width), "typestr": "<i4", "strides": (img.pitch_bytes, 4),
                                      "data": (img.data, False), "version": 2}
        return torch.as_tensor(h, device=device)
    dt = _FMT_TORCH[img.format]
    es = torch.empty((), dtype=dt).element_size()
    typestr = {torch.uint8: "|u1", torch.float16: "<f2", torch.float32: "<f4"}[dt]
    h.__cuda_array_interface__ = {"shape": (img.height, img.width, 4), "typestr": typestr,
                                  "strides": (img.pitch_bytes, 4 * es, es), "data": (img.data, False), "version": 2}
    return torch.as_tensor(h, device=device)
