"""nhwcodec_amd -- MI355X-native NHW encoder hot path.

Host-side mirror of the reference's C interface (rcanut/nhwcodec encoder/codec.h:184-219: quality setting in,
512x512 BGR24 image in, .nhw bytes out) over the C ABI of libnhwhip.so (include/nhw_hip.h).  PyTorch is
used only as plumbing: device buffers, streams, torch.distributed.  There is no CPU path: if the HIP
library is missing or no GPU is visible, construction fails.
"""
import ctypes
import math
import numbers
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libnhwhip.so")
IMG_BYTES = 786432
OUT_STRIDE = 512 << 10
QUALITY_DEFAULT = 20          # reference nhw_encoder_cli.c:95 (NORM)
# per-image / call status (include/nhw_hip.h)
NHW_OK, NHW_E_QUALITY, NHW_E_CODEBOOK, NHW_E_SPACE, NHW_E_ARG, NHW_E_HIP, NHW_E_FORMAT = 0, -1, -2, -3, -4, -5, -6
NHW_E_BUDGET = -7             # encode_fit*: no quality of the ladder fits the image's byte or distortion budget
PEAK_SSE_NUMERATOR = 65025 * IMG_BYTES   # 255^2 * 786432: PSNR = 10 log10(PEAK_SSE_NUMERATOR / SSE)

P = ctypes.c_void_p


class Timing(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("total_ms", "front_ms", "color_dwt_ms", "luma_ms", "chroma_ms", "entropy_ms")] + [("parts", ctypes.c_int), ("front_images", ctypes.c_int), ("prefilter_ms", ctypes.c_float)]


class FitStats(ctypes.Structure):
    """the last fit call (nhw_fit_stats): rungs run, quality and images encoded at each rung (ladder order), wall time"""
    _fields_ = [("rungs", ctypes.c_int), ("quality", ctypes.c_int * 23), ("images", ctypes.c_int * 23), ("total_ms", ctypes.c_float)]


class NhwError(RuntimeError):
    pass


class CTensorFormat(ctypes.Structure):
    """nhw_tensor_format (include/nhw_hip.h)"""
    _fields_ = [(n, ctypes.c_int32) for n in ("dtype", "layout", "channels", "rows")] + [("scale", ctypes.c_float * 3), ("bias", ctypes.c_float * 3), ("reserved", ctypes.c_uint32)]


def load_library(path: str = LIB_PATH) -> ctypes.CDLL:
    if not os.path.exists(path):
        raise NhwError(f"{path} not built: run `python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc); there is no CPU fallback")
    # torch brings its own HIP runtime; a process must have one.  Loaded after torch, libnhwhip.so binds to the runtime that is there; loaded
    # before it, the system's runtime comes in first and torch (or this library) then finds no device (`g.build(); g.smoke()` in one process).
    import torch  # noqa: F401
    L = ctypes.CDLL(path)
    L.nhw_last_error.restype = ctypes.c_char_p
    L.nhw_enc_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
    L.nhw_enc_create_ex.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.POINTER(P)]
    L.nhw_enc_destroy.argtypes = [P]
    L.nhw_quality_supported.argtypes = [ctypes.c_int]
    L.nhw_enc_set_compat.argtypes = [P, ctypes.c_int]
    L.nhw_enc_batch_device.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, P, P, P]
    L.nhw_enc_batch.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, ctypes.c_size_t, P, P]
    L.nhw_synth_batch_device.argtypes = [P, P, ctypes.c_int, ctypes.c_uint32, P]
    L.nhw_enc_last_timing.argtypes = [P, ctypes.POINTER(Timing)]
    L.nhw_enc_synth_batch.argtypes = [P, ctypes.c_int, ctypes.c_uint32, ctypes.c_int, P, ctypes.c_size_t, P, P]
    L.nhw_host_alloc.restype = P
    L.nhw_host_alloc.argtypes = [ctypes.c_size_t]
    L.nhw_host_free.argtypes = [P]
    L.nhw_device_count.restype = ctypes.c_int
    L.nhw_enc_fit_batch_device.argtypes = [P, P, ctypes.c_int, P, P, ctypes.c_int, P, P, P, P, P]
    L.nhw_enc_fit_batch.argtypes = [P, P, ctypes.c_int, P, P, ctypes.c_int, P, ctypes.c_size_t, P, P, P]
    L.nhw_enc_last_fit_stats.argtypes = [P, ctypes.POINTER(FitStats)]
    L.nhw_sse_batch_device.argtypes = [P, P, ctypes.c_int, P, P]
    L.nhw_enc_fit_sse_batch_device.argtypes = [P, P, P, ctypes.c_int, P, P, ctypes.c_int, P, P, P, P, P, P]
    L.nhw_enc_fit_sse_batch.argtypes = [P, P, P, ctypes.c_int, P, P, ctypes.c_int, P, ctypes.c_size_t, P, P, P, P]
    L.nhw_stage_color.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P, P, P, P]
    L.nhw_stage_prefilter.argtypes = [P, P, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_chroma_l1.argtypes = [P, ctypes.c_int, P]
    L.nhw_stage_chroma_loops.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_chroma_tail.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_luma_loop.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_ll2_walk.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_quant.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_residuals.argtypes = [P, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_stream.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P, P]
    L.nhw_debug_write.argtypes = [P, ctypes.c_int, ctypes.c_int, P, ctypes.c_size_t]
    L.nhw_stage_analysis.argtypes = [P, P, P, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_stage_synthesis.argtypes = [P, P, P, ctypes.c_int, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, P]
    L.nhw_debug_slice_order.argtypes = [P, ctypes.c_int]
    L.nhw_dec_debug_slice_order.argtypes = [P, ctypes.c_int]
    L.nhw_picture_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    L.nhw_tile_pictures_device.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P]
    L.nhw_untile_pictures_device.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_picture_info.argtypes = [P, ctypes.c_size_t, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.nhw_enc_pictures.argtypes = [P, P, P, P, P, ctypes.c_int, ctypes.c_int, P, ctypes.c_size_t, P, P]
    L.nhw_dec_pictures.argtypes = [P, P, P, ctypes.c_int, P, P, P]
    L.nhw_sse_pictures_device.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P, P]
    L.nhw_enc_fit_pictures.argtypes = [P, P, P, P, P, ctypes.c_int, P, P, ctypes.c_int, P, ctypes.c_size_t, P, P, P]
    L.nhw_enc_fit_sse_pictures.argtypes = [P, P, P, P, P, P, ctypes.c_int, P, P, ctypes.c_int, P, ctypes.c_size_t, P, P, P, P]
    L.nhw_region_tiles.argtypes = [ctypes.c_uint32] * 6
    L.nhw_untile_regions_device.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_dec_regions.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_int, P, P, P]
    L.nhw_dec_regions_to_device.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_int, P, P, P]
    L.nhw_dec_last_region_stats.argtypes = [P, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    L.nhw_dec_batch_device_scaled.argtypes = [P, P, P, P, ctypes.c_int, ctypes.c_int, P, P, P, P]
    L.nhw_dec_batch_scaled.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, P, P, P]
    L.nhw_picture_scaled_size.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)]
    L.nhw_untile_pictures_scaled_device.argtypes = [P, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_dec_pictures_scaled.argtypes = [P, P, P, ctypes.c_int, ctypes.c_int, P, P, P]
    L.nhw_window_tiles.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int] + [ctypes.c_uint32] * 4
    L.nhw_untile_windows_device.argtypes = [P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, P]
    L.nhw_dec_windows.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, P, P, P]
    L.nhw_dec_windows_to_device.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, P, P, P]
    L.nhw_dec_batch_device_tensor.argtypes = [P, P, P, P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CTensorFormat), P, P, P, P]
    L.nhw_bytes_to_tensor_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(CTensorFormat), P, P]
    L.nhw_tensor_to_bytes_device.argtypes = [P, ctypes.c_int, ctypes.POINTER(CTensorFormat), P, P]
    L.nhw_crop_scale.argtypes = [ctypes.c_uint32] * 4
    L.nhw_resize_to_tensor_device.argtypes = [P, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(CTensorFormat), P, P, P]
    L.nhw_dec_crops_to_device.argtypes = [P, P, P, ctypes.c_int, P, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.POINTER(CTensorFormat), P, P, P]
    L.nhw_enc_batch_device_tensor.argtypes = [P, P, ctypes.c_int, ctypes.POINTER(CTensorFormat), ctypes.c_int, P, P, P, P]
    L.nhw_tile_tensors_device.argtypes = [P, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(CTensorFormat), P, P]
    L.nhw_area_to_tensor_device.argtypes = L.nhw_resize_to_tensor_device.argtypes
    L.nhw_dec_crops_to_device_filter.argtypes = L.nhw_dec_crops_to_device.argtypes + [ctypes.c_int]
    a = L.nhw_resize_to_tensor_device.argtypes
    L.nhw_resample_to_tensor_device.argtypes = a[:4] + [ctypes.c_int] + a[4:]
    L.nhw_dec_crops_to_device_resample.argtypes = L.nhw_dec_crops_to_device_filter.argtypes
    L.nhw_enc_pictures_resized.argtypes = [P, P, P, P, P, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int, P, ctypes.c_size_t, P, P]
    L.nhw_warp_to_tensor_device.argtypes = L.nhw_resize_to_tensor_device.argtypes          # the table of warps where the flags are
    L.nhw_dec_warps_to_device.argtypes = L.nhw_dec_crops_to_device.argtypes
    L.nhw_debug_warp_row_limit.argtypes, L.nhw_debug_warp_row_limit.restype = [ctypes.c_int], None
    L.nhw_grey_table.argtypes = [ctypes.c_int, P]
    L.nhw_dec_batch_device_grey.argtypes = L.nhw_dec_batch_device_tensor.argtypes
    a = L.nhw_dec_batch_device_tensor.argtypes                                             # the same with flags, maps and tone tables: the three tables behind the format
    L.nhw_dec_batch_device_tensor_ops.argtypes = L.nhw_dec_batch_device_grey_ops.argtypes = a[:7] + [P, P, P] + a[7:]
    L.nhw_dec_batch_grey.argtypes = L.nhw_dec_batch_scaled.argtypes
    L.nhw_untile_windows_grey_device.argtypes = L.nhw_untile_windows_device.argtypes       # the grey calls: their colour calls' arguments
    L.nhw_resample_grey_to_tensor_device.argtypes = L.nhw_resample_to_tensor_device.argtypes
    L.nhw_warp_grey_to_tensor_device.argtypes = L.nhw_warp_to_tensor_device.argtypes
    L.nhw_dec_windows_grey.argtypes = L.nhw_dec_windows.argtypes
    L.nhw_dec_windows_grey_to_device.argtypes = L.nhw_dec_windows_to_device.argtypes
    L.nhw_dec_crops_grey_to_device.argtypes = L.nhw_dec_crops_to_device_resample.argtypes
    L.nhw_dec_warps_grey_to_device.argtypes = L.nhw_dec_warps_to_device.argtypes
    a = L.nhw_resample_to_tensor_device.argtypes                                           # the mapped calls: the table of maps behind the flags or warps
    L.nhw_resample_mapped_to_tensor_device.argtypes = a[:7] + [P] + a[7:]
    a = L.nhw_warp_to_tensor_device.argtypes
    L.nhw_warp_mapped_to_tensor_device.argtypes = a[:6] + [P] + a[6:]
    a = L.nhw_dec_crops_to_device_resample.argtypes
    L.nhw_dec_crops_mapped_to_device.argtypes = a[:11] + [P] + a[11:]
    a = L.nhw_dec_warps_to_device.argtypes
    L.nhw_dec_warps_mapped_to_device.argtypes = a[:11] + [P] + a[11:]
    a = L.nhw_resample_mapped_to_tensor_device.argtypes                                    # the toned calls: the table of tone tables behind the maps
    L.nhw_resample_toned_to_tensor_device.argtypes = a[:8] + [P] + a[8:]
    a = L.nhw_warp_mapped_to_tensor_device.argtypes
    L.nhw_warp_toned_to_tensor_device.argtypes = a[:7] + [P] + a[7:]
    a = L.nhw_dec_crops_mapped_to_device.argtypes
    L.nhw_dec_crops_toned_to_device.argtypes = a[:12] + [P] + a[12:]
    a = L.nhw_dec_warps_mapped_to_device.argtypes
    L.nhw_dec_warps_toned_to_device.argtypes = a[:12] + [P] + a[12:]
    L.nhw_hist_device.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P]
    L.nhw_grey_luma_table.argtypes = [ctypes.c_int, P]                                     # encode grey: their colour calls' arguments
    L.nhw_enc_batch_device_grey.argtypes = L.nhw_enc_batch_device.argtypes
    L.nhw_enc_batch_grey.argtypes = L.nhw_enc_batch.argtypes
    L.nhw_tensor_to_bytes_grey_device.argtypes = L.nhw_tensor_to_bytes_device.argtypes
    L.nhw_enc_batch_device_grey_tensor.argtypes = L.nhw_enc_batch_device_tensor.argtypes
    L.nhw_tile_pictures_grey_device.argtypes = L.nhw_tile_pictures_device.argtypes
    L.nhw_enc_pictures_grey.argtypes = L.nhw_enc_pictures.argtypes
    L.nhw_tone_from_hist_device.argtypes = [P, ctypes.c_int, ctypes.c_int, P, P, P]
    return L


_LIB = None


def _library():
    global _LIB
    if _LIB is None:
        _LIB = load_library()
    return _LIB


def psnr_to_max_sse(db):
    """the largest SSE whose PSNR is at least `db`: floor(65025 * 786432 * 10**(-db/10)) in float64, for finite db > 0.  A number gives an int,
    an array (or list) of them an int64 numpy array."""
    import numpy as np
    try:
        a = np.asarray(db, dtype=np.float64)
    except (TypeError, ValueError):
        raise NhwError(f"a PSNR target must be a finite number of dB above 0, got {db!r}") from None
    if a.size == 0 or not np.all(np.isfinite(a)) or not np.all(a > 0):
        raise NhwError(f"a PSNR target must be a finite number of dB above 0, got {db!r}")
    m = np.floor(float(PEAK_SSE_NUMERATOR) * np.power(10.0, -a / 10.0)).astype(np.int64)
    return int(m) if m.ndim == 0 else m


def sse_device(a, b):
    """The exact sum of squared differences of every picture of `a` against the same picture of `b` (nhw_sse_batch_device): two contiguous
    uint8 CUDA tensors of n * 786432 bytes each (e.g. [n, 512, 512, 3]) on one device, 16-byte aligned -> int64 tensor [n] on that device.
    Ordered on torch's current stream."""
    import torch
    for name, x in (("a", a), ("b", b)):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and x.is_contiguous() and x.numel() > 0 and x.numel() % IMG_BYTES == 0):
            raise NhwError(f"sse_device: `{name}` must be a contiguous uint8 CUDA tensor of n * {IMG_BYTES} bytes")
    if a.numel() != b.numel() or a.device != b.device:
        raise NhwError("sse_device: `a` and `b` must hold as many pictures, on one device")
    n = a.numel() // IMG_BYTES
    L = _library()
    out = torch.empty(n, dtype=torch.int64, device=a.device)
    with torch.cuda.device(a.device):
        rc = L.nhw_sse_batch_device(a.data_ptr(), b.data_ptr(), n, out.data_ptr(), torch.cuda.current_stream(a.device).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


# ---------------------------------------------------------------- pictures of any size as padded tiles
PICTURE_DTYPE = [("addr", "<u8"), ("pitch", "<u8"), ("width", "<u4"), ("height", "<u4"), ("first_tile", "<u4"), ("reserved", "<u4")]   # nhw_picture


def picture_tiles(width: int, height: int) -> int:
    """ceil(width / 512) * ceil(height / 512): the tiles of a width x height picture (sides 1..65535)"""
    if not (1 <= width <= 65535 and 1 <= height <= 65535):
        raise NhwError(f"a picture side must be 1..65535, got {width} x {height}")
    return ((width + 511) // 512) * ((height + 511) // 512)


# ---------------------------------------------------------------- half and quarter scale
SCALES = (1, 2, 4)


def _scale(scale, what):
    if isinstance(scale, bool) or not isinstance(scale, numbers.Integral) or scale not in SCALES:
        raise NhwError(f"{what}: the scale must be 1, 2 or 4, got {scale!r}")
    return int(scale)


def scaled_size(width: int, height: int, scale: int) -> tuple:
    """(ceil(width / scale), ceil(height / scale)): the size of a width x height picture (sides 1..65535) decoded at scale 1, 2 or 4.  Its tiles
    have the side 512 // scale and are as many as the whole picture's."""
    scale = _scale(scale, "scaled_size")
    if not (isinstance(width, numbers.Integral) and isinstance(height, numbers.Integral)):
        raise NhwError(f"a picture's sides must be integers, got {width!r} x {height!r}")
    picture_tiles(int(width), int(height))
    return -(-int(width) // scale), -(-int(height) // scale)


# ---------------------------------------------------------------- a rectangle of a picture from the tiles it touches
REGION_DTYPE = [("addr", "<u8"), ("pitch", "<u8"), ("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4"), ("pic_width", "<u4"),
                ("pic_height", "<u4"), ("first_tile", "<u4"), ("reserved", "<u4")]   # nhw_region
RECT_DTYPE = [("container", "<u4"), ("x", "<u4"), ("y", "<u4"), ("width", "<u4"), ("height", "<u4")]   # nhw_rect


def region_tiles(pic_width: int, pic_height: int, x: int, y: int, width: int, height: int) -> int:
    """the tiles the region x, y, width, height of a pic_width x pic_height picture selects (nhw_region_tiles): columns x // 512 ..
    (x + width - 1) // 512 times rows y // 512 .. (y + height - 1) // 512"""
    picture_tiles(pic_width, pic_height)
    if not (width >= 1 and height >= 1 and x >= 0 and y >= 0 and x + width <= pic_width and y + height <= pic_height):
        raise NhwError(f"the region {x}, {y}, {width} x {height} is empty or not inside the {pic_width} x {pic_height} picture")
    return ((x + width - 1) // 512 - x // 512 + 1) * ((y + height - 1) // 512 - y // 512 + 1)


WINDOW_USE_DTYPE = [("region", "<u4"), ("slot", "<u4"), ("tx", "<u4"), ("ty", "<u4")]   # nhw_window_use


def window_tiles(pic_width: int, pic_height: int, scale: int, x: int, y: int, width: int, height: int) -> int:
    """the tiles the window x, y, width, height of a pic_width x pic_height picture at scale 1, 2 or 4 selects (nhw_window_tiles, DESIGN.md
    section 15): the rectangle is in the coordinates of the scaled picture (scaled_size), whose tiles have the side T = 512 // scale: columns
    x // T .. (x + width - 1) // T times rows y // T .. (y + height - 1) // T.  At scale 1 it is region_tiles."""
    scale = _scale(scale, "window_tiles")
    sw, sh = scaled_size(pic_width, pic_height, scale)
    if not (width >= 1 and height >= 1 and x >= 0 and y >= 0 and x + width <= sw and y + height <= sh):
        raise NhwError(f"the window {x}, {y}, {width} x {height} is empty or not inside the {sw} x {sh} picture ({pic_width} x {pic_height} at scale {scale})")
    side = 512 // scale
    return ((x + width - 1) // side - x // side + 1) * ((y + height - 1) // side - y // side + 1)


# ---------------------------------------------------------------- decode straight into training tensors
NHW_T_U8, NHW_T_F16, NHW_T_BF16, NHW_T_F32 = 0, 1, 2, 3
TENSOR_DTYPES = {"uint8": NHW_T_U8, "float16": NHW_T_F16, "bfloat16": NHW_T_BF16, "float32": NHW_T_F32}
TENSOR_LAYOUTS = {"HWC": 0, "CHW": 1}             # NHW_T_HWC, NHW_T_CHW
TENSOR_CHANNELS = {"BGR": 0, "RGB": 1}            # NHW_T_BGR, NHW_T_RGB
TENSOR_GREY = 2                                   # NHW_T_GREY: channels "GREY", which the grey decode and the grey calls alone take (DESIGN.md sections 22, 23)
TENSOR_ROWS = {"file": 0, "reversed": 1}          # NHW_T_ROWS_FILE, NHW_T_ROWS_REVERSED


class TensorFormat:
    """The form decoded pixels leave in (nhw_tensor_format): dtype torch.uint8 / float16 / bfloat16 / float32 (or its name), layout "CHW"
    ([3, S, S]) or "HWC" ([S, S, 3], as the byte path), channels "RGB" or "BGR" (as the byte path), rows "file" (BMP file order, bottom-up,
    as the byte path) or "reversed" (top-down: row 0 is the picture's top row), and per OUTPUT channel a scale and a bias: the element for
    byte b of channel c is fmaf(float32(b), scale[c], bias[c]) in single precision, rounded once to dtype.  uint8 passes the bytes on and
    takes scale 1, bias 0 only.  The rounding to dtype comes after the fma's own rounding to float32: two roundings in all, both to nearest
    even, and that two-step result is the rule (on rare values it is not the exact b * scale + bias rounded once to dtype).  Subnormals
    are kept and overflow gives an infinity, in float32 and in dtype.  Zero's sign is the fma's: a nonzero value that rounds to zero keeps
    its sign; an exact zero is +0, except -0 for a zero product of negative sign (byte 0 under a scale below zero) plus a bias of -0.0.  Either scale / bias (three numbers each, or one for all; default 1 and 0) or mean / std in units of 0..1
    pixels, which give, in float32 arithmetic, scale = 1 / (255 * std) and bias = -mean / std (so that the element is (b / 255 - mean) / std
    up to rounding).  The attributes scale and bias are the float32 constants the kernels get, as tuples of Python floats.
    channels "GREY" is the one-channel format of Decoder.decode_grey_device and of the calls with `grey` in their names
    (section 23), and of nothing else: scale / bias / mean /
    std take ONE number (three are refused), the tensor is [1, S, S] or [S, S, 1], and its inverse is inverted_grey(), which the grey
    encode calls take (section 27)."""

    def __init__(self, dtype="float32", layout="CHW", channels="RGB", rows="reversed", scale=None, bias=None, mean=None, std=None):
        import numpy as np
        name = dtype if isinstance(dtype, str) else str(dtype).replace("torch.", "")
        if name not in TENSOR_DTYPES:
            raise NhwError(f"TensorFormat: dtype must be uint8, float16, bfloat16 or float32, got {dtype!r}")
        for what, v, table in (("layout", layout, TENSOR_LAYOUTS), ("channels", channels, dict(TENSOR_CHANNELS, GREY=TENSOR_GREY)), ("rows", rows, TENSOR_ROWS)):
            if not isinstance(v, str) or v not in table:
                raise NhwError(f"TensorFormat: {what} must be one of {sorted(table)}, got {v!r}")
        if (mean is not None or std is not None) and (scale is not None or bias is not None):
            raise NhwError("TensorFormat: give scale / bias or mean / std, not both")

        def three(v, default, what):
            if v is None:
                v = default
            try:
                with np.errstate(over="ignore"):
                    a = np.asarray(v, dtype=np.float64).astype(np.float32)
            except (TypeError, ValueError):
                raise NhwError(f"TensorFormat: {what} must be one number or three, got {v!r}") from None
            if channels == "GREY" and a.ndim != 0:
                raise NhwError(f"TensorFormat: with channels \"GREY\" {what} must be one number, got {v!r}")
            if a.ndim == 0:
                a = np.repeat(a, 3)
            if a.shape != (3,):
                raise NhwError(f"TensorFormat: {what} must be one number or three, got {v!r}")
            if not np.all(np.isfinite(a)):
                raise NhwError(f"TensorFormat: {what} must be finite in float32, got {v!r}")
            return a

        if mean is not None or std is not None:
            m, sd = three(mean, 0.0, "mean"), three(std, 1.0, "std")
            with np.errstate(all="ignore"):
                sc = np.float32(1) / (np.float32(255) * sd)
                bi = -m / sd
            if not (np.all(np.isfinite(sc)) and np.all(np.isfinite(bi))):
                raise NhwError(f"TensorFormat: mean {mean!r} / std {std!r} give no finite float32 scale and bias")
        else:
            sc, bi = three(scale, 1.0, "scale"), three(bias, 0.0, "bias")
        if name == "uint8" and not (np.all(sc == 1) and np.all(bi == 0)):
            raise NhwError("TensorFormat: uint8 passes the bytes on: scale must be 1 and bias 0")
        self.dtype_name, self.layout, self.channels, self.rows = name, layout, channels, rows
        self.scale = tuple(float(x) for x in sc)
        self.bias = tuple(float(x) for x in bi)

    @property
    def dtype(self):
        import torch
        return getattr(torch, self.dtype_name)

    def shape(self, height, width):
        """the shape of one picture's tensor"""
        c = 1 if self.channels == "GREY" else 3
        return (c, height, width) if self.layout == "CHW" else (height, width, c)

    def c_struct(self) -> CTensorFormat:
        return CTensorFormat(TENSOR_DTYPES[self.dtype_name], TENSOR_LAYOUTS[self.layout], TENSOR_GREY if self.channels == "GREY" else TENSOR_CHANNELS[self.channels], TENSOR_ROWS[self.rows],
                             (ctypes.c_float * 3)(*self.scale), (ctypes.c_float * 3)(*self.bias), 0)

    def inverted(self):
        """The format that ENCODES what a decode under this one produced: the same dtype, layout, channels and rows, and in float32 arithmetic
        scale' = 1 / scale and bias' = -bias / scale, so that fmaf(fmaf(b, scale, bias), scale', bias') lies near b.  NhwError if a scale is 0 or
        a result is not finite in float32."""
        import numpy as np
        if self.channels == "GREY":
            raise NhwError("TensorFormat.inverted: a grey format is inverted by inverted_grey(), for the grey encode calls")
        sc, bi = np.array(self.scale, np.float32), np.array(self.bias, np.float32)
        if np.any(sc == 0):
            raise NhwError(f"TensorFormat.inverted: a scale of 0 has no inverse: {self.scale}")
        with np.errstate(all="ignore"):
            isc, ibi = np.float32(1) / sc, -bi / sc
        if not (np.all(np.isfinite(isc)) and np.all(np.isfinite(ibi))):
            raise NhwError(f"TensorFormat.inverted: scale {self.scale} / bias {self.bias} give no finite float32 inverse")
        return TensorFormat(self.dtype_name, self.layout, self.channels, self.rows, scale=tuple(float(x) for x in isc), bias=tuple(float(x) + 0.0 for x in ibi))

    def inverted_grey(self):
        """inverted() for a format of channels "GREY": the format that encodes, through the grey encode calls, what a grey
        decode under this one produced -- the same dtype, layout and rows, and in float32 arithmetic scale' = 1 / scale, bias' = -bias / scale on
        the one scale and bias.  NhwError for a colour format, a scale of 0 or a result that is not finite in float32."""
        import numpy as np
        if self.channels != "GREY":
            raise NhwError(f"TensorFormat.inverted_grey: the format has channels {self.channels!r}, not \"GREY\": inverted() is its inverse")
        sc, bi = np.float32(self.scale[0]), np.float32(self.bias[0])
        if sc == 0:
            raise NhwError(f"TensorFormat.inverted_grey: a scale of 0 has no inverse: {self.scale[0]}")
        with np.errstate(all="ignore"):
            isc, ibi = np.float32(1) / sc, -bi / sc
        if not (np.isfinite(isc) and np.isfinite(ibi)):
            raise NhwError(f"TensorFormat.inverted_grey: scale {self.scale[0]} / bias {self.bias[0]} give no finite float32 inverse")
        return TensorFormat(self.dtype_name, self.layout, "GREY", self.rows, scale=float(isc), bias=float(ibi) + 0.0)

    def __repr__(self):
        return f"TensorFormat({self.dtype_name}, {self.layout}, {self.channels}, rows={self.rows}, scale={self.scale}, bias={self.bias})"


def grey_table(quality: int):
    """G_quality (nhw_grey_table): numpy uint8 [256], the grey byte of every luma byte under the colour matrix of that
    quality at neutral chroma -- the identity for quality 20 .. 23, a gain curve below.  Needs no GPU."""
    import numpy as np
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 23:
        raise NhwError(f"grey_table: quality must be an integer 1 .. 23, got {quality!r}")
    t = np.empty(256, np.uint8)
    if _library().nhw_grey_table(quality, t.ctypes.data) != 0:
        raise NhwError(f"grey_table: {_library().nhw_dec_last_error().decode()}")
    return t


def grey_luma_table(quality: int):
    """L_quality (nhw_grey_luma_table): numpy int16 [256], the encoder's luma of the pixel B = G = R = g under that
    quality -- the identity for quality 20 .. 23, the byte scaled for 17 .. 19, the integer form from 16 down.  Needs no GPU."""
    import numpy as np
    if isinstance(quality, bool) or not isinstance(quality, int) or not 1 <= quality <= 23:
        raise NhwError(f"grey_luma_table: quality must be an integer 1 .. 23, got {quality!r}")
    t = np.empty(256, np.int16)
    if _library().nhw_grey_luma_table(quality, t.ctypes.data) != 0:
        raise NhwError(f"grey_luma_table: {_library().nhw_last_error().decode()}")
    return t


def _tensor_format(fmt, what, grey=False):
    """the checked format of a call: a TensorFormat, of channels "GREY" for a grey call (grey=True) and of no such for a colour call (False);
    None: either"""
    if not isinstance(fmt, TensorFormat):
        raise NhwError(f"{what}: `fmt` must be a TensorFormat, got {type(fmt).__name__}")
    if grey is True and fmt.channels != "GREY":
        raise NhwError(f"{what}: `fmt` must have channels \"GREY\", got {fmt.channels!r}")
    if grey is False and fmt.channels == "GREY":
        raise NhwError(f"{what}: `fmt` has channels \"GREY\", which the grey calls alone take")
    return fmt


def _picture_table(pictures, what, side=512, channels=3):
    """the checked nhw_picture table of a list of uint8 CUDA tensors [H, W, 3] with strides (pitch, 3, 1), on one device -> (table as an
    int64 CUDA tensor, total tiles, device).  side: the tile side (512; 256 or 128 for the pictures of a scaled decode).  channels=1: the
    one-byte pictures of the grey calls, [H, W] with strides (pitch >= W, 1)"""
    import numpy as np
    import torch
    C = channels
    form = "[H, W, 3]" if C == 3 else "[H, W]"
    if not isinstance(pictures, (list, tuple)) or not pictures:
        raise NhwError(f"{what} wants a non-empty list of uint8 CUDA tensors {form}")
    dev = pictures[0].device if isinstance(pictures[0], torch.Tensor) else None
    table = np.zeros(len(pictures), PICTURE_DTYPE)
    tiles = 0
    for i, x in enumerate(pictures):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.uint8 and (x.dim() == 3 and x.shape[2] == 3 if C == 3 else x.dim() == 2)):
            raise NhwError(f"{what}: picture {i} is not a uint8 CUDA tensor {form}")
        if x.device != dev:
            raise NhwError(f"{what}: picture {i} is on {x.device}, picture 0 on {dev}")
        h, w = int(x.shape[0]), int(x.shape[1])
        t = picture_tiles(w, h) if side == 512 else (-(-w // side)) * (-(-h // side))
        if C == 1 and ((w > 1 and x.stride(1) != 1) or (h > 1 and x.stride(0) < w)):
            raise NhwError(f"{what}: picture {i} must have strides (pitch >= W, 1), got {tuple(x.stride())}")
        if C == 3 and (x.stride(2) != 1 or (w > 1 and x.stride(1) != 3) or (h > 1 and x.stride(0) < 3 * w)):
            raise NhwError(f"{what}: picture {i} must have strides (pitch >= 3 W, 3, 1), got {tuple(x.stride())}")
        table[i] = (x.data_ptr(), x.stride(0) if h > 1 else C * w, w, h, tiles, 0)
        tiles += t
    return torch.from_numpy(table.view(np.int64).copy()).to(dev), tiles, dev


def tile_pictures_device(pictures):
    """Pad every picture to whole 512 x 512 tiles by edge replication and cut the tiles out on the device (k_tile_pad): a list of uint8 CUDA
    tensors [H, W, 3] (BMP file row order) on one device, rows any pitch (crop views of a larger tensor work without a copy) -> tiles uint8
    [T, 512, 512, 3], picture after picture, each row-major.  Ordered on torch's current stream; feeds Encoder.encode_device."""
    import torch
    table, tiles, dev = _picture_table(pictures, "tile_pictures_device")
    out = torch.empty((tiles, 512, 512, 3), dtype=torch.uint8, device=dev)
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_tile_pictures_device(table.data_ptr(), len(pictures), 0, tiles, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def tile_pictures_grey_device(pictures):
    """tile_pictures_device at one byte a pixel (nhw_tile_pictures_grey_device): a list of uint8 CUDA tensors [H, W] with
    strides (pitch >= W, 1) on one device (crop views work without a copy) -> tiles uint8 [T, 512, 512], padded by edge replication.  Ordered on
    torch's current stream; feeds Encoder.encode_grey_device."""
    import torch
    table, tiles, dev = _picture_table(pictures, "tile_pictures_grey_device", channels=1)
    out = torch.empty((tiles, 512, 512), dtype=torch.uint8, device=dev)
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_tile_pictures_grey_device(table.data_ptr(), len(pictures), 0, tiles, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def _picture_tiles_arg(tiles, pictures, what):
    """the checked table of `pictures` (as for tile_pictures_device) and `tiles`, a contiguous uint8 tensor of all their tiles on their device"""
    import torch
    table, n_tiles, dev = _picture_table(pictures, what)
    if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.device == dev and tiles.dtype == torch.uint8 and tiles.is_contiguous()
            and tiles.numel() == n_tiles * IMG_BYTES):
        raise NhwError(f"{what}: `tiles` must be a contiguous uint8 tensor [{n_tiles}, 512, 512, 3] on {dev}")
    return table, n_tiles, dev


def untile_pictures_device(tiles, pictures):
    """The inverse of tile_pictures_device (k_untile_crop): decoded tiles uint8 [T, 512, 512, 3] (e.g. Decoder.decode_device's pixels) into
    the preallocated pictures (as for tile_pictures_device); only the pictures' own bytes are written.  Ordered on torch's current stream."""
    import torch
    table, n_tiles, dev = _picture_tiles_arg(tiles, pictures, "untile_pictures_device")
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_untile_pictures_device(tiles.data_ptr(), table.data_ptr(), len(pictures), 0, n_tiles, torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")


def untile_scaled_pictures_device(tiles, pictures, scale):
    """untile_pictures_device for the tiles of a scaled decode (nhw_untile_pictures_scaled_device): tiles uint8 [T, S, S, 3] with S = 512 // scale
    (e.g. Decoder.decode_scaled_device's pixels) into the preallocated pictures, given as for untile_pictures_device but at their SCALED sizes
    (scaled_size); picture k takes ceil(W' / S) * ceil(H' / S) tiles.  Only the pictures' own bytes are written.  Ordered on torch's current stream."""
    import torch
    what = "untile_scaled_pictures_device"
    scale = _scale(scale, what)
    side = 512 // scale
    if isinstance(pictures, (list, tuple)):
        for i, x in enumerate(pictures):
            if isinstance(x, torch.Tensor) and x.dim() == 3 and not (1 <= x.shape[0] <= -(-65535 // scale) and 1 <= x.shape[1] <= -(-65535 // scale)):
                raise NhwError(f"{what}: picture {i} is {x.shape[1]} x {x.shape[0]}, beyond a 65535 x 65535 picture at scale {scale}")
    table, n_tiles, dev = _picture_table(pictures, what, side)
    if not (isinstance(tiles, torch.Tensor) and tiles.is_cuda and tiles.device == dev and tiles.dtype == torch.uint8 and tiles.is_contiguous()
            and tiles.numel() == n_tiles * 3 * side * side):
        raise NhwError(f"{what}: `tiles` must be a contiguous uint8 tensor [{n_tiles}, {side}, {side}, 3] on {dev}")
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_untile_pictures_scaled_device(tiles.data_ptr(), table.data_ptr(), len(pictures), 0, n_tiles, scale, torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")


def pictures_to_tensor_device(pictures, fmt):
    """What is already bytes, to a tensor format in one pass (k_bytes_to_tensor, nhw_bytes_to_tensor_device): a list of uint8 CUDA tensors
    [H, W, 3] as for tile_pictures_device (any size, any pitch: the outputs of decode_pictures*, of the region and window calls, crop views)
    -> a list of new tensors of fmt.dtype, [3, H, W] or [H, W, 3] each, under TensorFormat's value rule.  Reads only the pictures' own bytes.
    Ordered on torch's current stream."""
    import numpy as np
    import torch
    what = "pictures_to_tensor_device"
    fmt = _tensor_format(fmt, what)
    table, _, dev = _picture_table(pictures, what)
    outs = [torch.empty(fmt.shape(int(x.shape[0]), int(x.shape[1])), dtype=fmt.dtype, device=dev) for x in pictures]
    addr = torch.from_numpy(np.array([o.data_ptr() for o in outs], dtype=np.uint64).view(np.int64)).to(dev)
    L = _library()
    c = fmt.c_struct()
    with torch.cuda.device(dev):
        rc = L.nhw_bytes_to_tensor_device(table.data_ptr(), len(pictures), ctypes.byref(c), addr.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return outs


# ---------------------------------------------------------------- crops resized into tensors of one size
CROP_SIDE_MAX = 4096


def _crop_size(size, what):
    """the checked (out_h, out_w) of a crop call"""
    if not (isinstance(size, (tuple, list)) and len(size) == 2 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in size)
            and all(1 <= v <= CROP_SIDE_MAX for v in size)):
        raise NhwError(f"{what}: `size` must be (out_h, out_w), integers of 1 .. {CROP_SIDE_MAX}, got {size!r}")
    return int(size[0]), int(size[1])


def _crop_flips(flips, n, what):
    """the flag bytes of n crops (bit 0: mirror left-right) as a numpy uint8 array, or None"""
    import numpy as np
    if flips is None:
        return None
    try:
        f = np.asarray(flips)
    except Exception:
        f = None
    if f is None or f.shape != (n,) or f.dtype.kind not in "biu":
        raise NhwError(f"{what}: `flips` must be {n} booleans or flag bytes, one a crop, got {flips!r}")
    return np.ascontiguousarray(f.astype(bool).astype(np.uint8) if f.dtype.kind == "b" else (f & 1).astype(np.uint8))


def crop_scale(w: int, h: int, out_w: int, out_h: int) -> int:
    """the scale to decode a w x h crop at that goes to out_w x out_h (nhw_crop_scale): the largest s of 4, 2, 1 with s * out_w <= w and
    s * out_h <= h, which leaves the two-tap resize a reduction below 2; 1 if there is none (the crop is enlarged)"""
    if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (w, h, out_w, out_h)):
        raise NhwError(f"crop_scale wants integers, got {(w, h, out_w, out_h)!r}")
    if not (1 <= w <= 0xFFFFFFFF and 1 <= h <= 0xFFFFFFFF and 1 <= out_w <= CROP_SIDE_MAX and 1 <= out_h <= CROP_SIDE_MAX):
        raise NhwError(f"crop_scale: a {w} x {h} crop to {out_w} x {out_h}: the sides must be at least 1, the output's {CROP_SIDE_MAX} at the most")
    for s in (4, 2):
        if s * out_w <= w and s * out_h <= h:
            return s
    return 1


def crop_window(x: int, y: int, w: int, h: int, scale: int) -> tuple:
    """the smallest window at `scale` that covers the full-resolution crop x, y, w, h -> (x', y', w', h') with x' = x // s, y' = y // s,
    w' = ceil((x + w) / s) - x', h' = ceil((y + h) / s) - y'.  A crop inside a W x H picture gives a window inside scaled_size(W, H, scale)."""
    scale = _scale(scale, "crop_window")
    if not all(isinstance(v, numbers.Integral) and not isinstance(v, bool) for v in (x, y, w, h)) or x < 0 or y < 0 or w < 1 or h < 1:
        raise NhwError(f"crop_window: the crop {x!r}, {y!r}, {w!r} x {h!r} is empty or no rectangle of integers")
    x, y, w, h = int(x), int(y), int(w), int(h)
    return x // scale, y // scale, -(-(x + w) // scale) - x // scale, -(-(y + h) // scale) - y // scale


RESAMPLERS = {"two_tap": 0, "area": 1, "cubic": 2}  # NHW_FILTER_TWO_TAP, NHW_FILTER_AREA, NHW_FILTER_CUBIC: what the `filter` arguments take
FILTERS = {k: v for k, v in RESAMPLERS.items() if k != "cubic"}   # ... without the cubic filter: what nhw_dec_crops_to_device_filter takes
AREA_MAX_REDUCTION = 128                           # NHW_AREA_MAX_REDUCTION: the area filter takes a side down to 1 / 128 at the most
CUBIC_MAX_REDUCTION = 32                           # NHW_CUBIC_MAX_REDUCTION: the cubic filter takes a side down to 1 / 32 at the most
_LIMITS = {"area": AREA_MAX_REDUCTION, "cubic": CUBIC_MAX_REDUCTION}   # the reduction limit by filter name; the two taps have none


def _filter(filter, what):
    """raises unless `filter` is a filter's name, a key of RESAMPLERS"""
    if not isinstance(filter, str) or filter not in RESAMPLERS:
        raise NhwError(f"{what}: `filter` must be one of {', '.join(repr(k) for k in RESAMPLERS)}, got {filter!r}")


def _filter_limit(filter, w, h, out_w, out_h, what, which):
    """raises for a picture or window beyond the reduction limit of the filter (a checked name)"""
    limit = _LIMITS.get(filter)
    if limit and (w > limit * out_w or h > limit * out_h):
        raise NhwError(f"{what}: {which} is {w} x {h}, more than {limit} times the output's {out_w} x {out_h} along a side: beyond the {filter} filter's limit")


_SAMPLE_ENTRIES = {   # kind: the C entry of a plain colour call, of a plain grey one, of a mapped and of a toned one (either family, by the format)
    "resample": ("nhw_resample_to_tensor_device", "nhw_resample_grey_to_tensor_device", "nhw_resample_mapped_to_tensor_device", "nhw_resample_toned_to_tensor_device"),
    "warp": ("nhw_warp_to_tensor_device", "nhw_warp_grey_to_tensor_device", "nhw_warp_mapped_to_tensor_device", "nhw_warp_toned_to_tensor_device"),
    "crops": ("nhw_dec_crops_to_device_resample", "nhw_dec_crops_grey_to_device", "nhw_dec_crops_mapped_to_device", "nhw_dec_crops_toned_to_device"),
    "warps": ("nhw_dec_warps_to_device", "nhw_dec_warps_grey_to_device", "nhw_dec_warps_mapped_to_device", "nhw_dec_warps_toned_to_device"),
}


def _sample_entry(lib, kind, channels, colours, tones):
    """the C entry of a sampling call and its table arguments, which go in front of the output addresses: with tone tables the toned entry, the
    maps (or None) and the tables; with maps alone the mapped entry and the maps; else the plain entry of the family and nothing"""
    colour, grey, mapped, toned = _SAMPLE_ENTRIES[kind]
    if tones is not None:
        return getattr(lib, toned), (colours, tones)
    if colours is not None:
        return getattr(lib, mapped), (colours,)
    return getattr(lib, colour if channels == 3 else grey), ()


def resize_to_tensor_device(pictures, size, fmt, flips=None, filter="two_tap", colours=None, tones=None):
    """Pictures of any sizes to one batch tensor of one size (k_resize_to_tensor, nhw_resize_to_tensor_device): a list of uint8 CUDA tensors
    [H, W, 3] as for pictures_to_tensor_device, size = (out_h, out_w) of 1 .. 4096 each, flips: None or one boolean a picture ("mirror
    left-right") -> a new tensor [n, 3, out_h, out_w] or [n, out_h, out_w, 3] of fmt.dtype.  Picture k is resampled under the integer rule
    of DESIGN.md section 18 (centre-aligned, two taps a direction, weights in 1/256), mirrored, and converted under TensorFormat's value
    rule.  filter="area" (k_area_to_tensor, nhw_area_to_tensor_device): an axis that shrinks takes the exact box mean
    instead, which does not alias; a picture more than AREA_MAX_REDUCTION times the output along a side is refused.  filter="cubic"
    (k_cubic_to_tensor, nhw_resample_to_tensor_device): the Keys cubic with a = -1/2, widened with the reduction, what
    PIL's BICUBIC and torch's antialiased bicubic compute, as an integer rule; the limit is CUBIC_MAX_REDUCTION.  Reads only the
    pictures' own bytes.  Ordered on torch's current stream.  colours: None, or one colour map a picture (nhw_resample_mapped_to_tensor_device,
    DESIGN.md section 24) -- a 3 x 4 matrix of floats on (R, G, B, 1) as colour_matrix makes it, or the twelve integers of colour_fixed --, applied
    to the resampled bytes in front of the value rule: y = clamp((m x + o + 1/2) floored), in 1/65536.  tones: None, or one tone table a picture
    (nhw_resample_toned_to_tensor_device) -- uint8 [3, 256] on R, G, B as the tone_* builders make it --, or a uint8 CUDA tensor
    [n, 768] in the struct's own order, as tone_from_hist_device returns it; the table acts on the bytes behind the map: z = t[y].  colours and
    tones combine."""
    return _resize_to_tensor("resize_to_tensor_device", 3, pictures, size, fmt, flips, filter, colours, tones)


def resize_grey_to_tensor_device(pictures, size, fmt, flips=None, filter="two_tap", colours=None, tones=None):
    """resize_to_tensor_device for one-channel pictures (nhw_resample_grey_to_tensor_device): a list of uint8 CUDA
    tensors [H, W] with strides (pitch >= W, 1), fmt a TensorFormat of channels "GREY" -> a new tensor [n, 1, out_h, out_w] or [n, out_h,
    out_w, 1] of fmt.dtype.  The rules of the three filters on the one channel; the value rule with the format's one scale and bias.  colours: None, or
    one pair (gain, offset) a picture, the one-channel form of resize_to_tensor_device's maps.  tones: None, or one table uint8 [256] a picture (or
    the CUDA tensor [n, 768], of which a sample's first 256 bytes are read)."""
    return _resize_to_tensor("resize_grey_to_tensor_device", 1, pictures, size, fmt, flips, filter, colours, tones)


def _resize_to_tensor(what, channels, pictures, size, fmt, flips, filter, colours=None, tones=None):
    """resize_to_tensor_device (channels=3) and resize_grey_to_tensor_device (1)"""
    import torch
    _filter(filter, what)
    fmt = _tensor_format(fmt, what, grey=channels == 1)
    out_h, out_w = _crop_size(size, what)
    if isinstance(pictures, (list, tuple)):                          # the limit from the shapes alone, before a device is looked at
        for i, x in enumerate(pictures):
            if len(getattr(x, "shape", ())) == (3 if channels == 3 else 2):
                _filter_limit(filter, int(x.shape[1]), int(x.shape[0]), out_w, out_h, what, f"picture {i}")
        maps = _colour_table(colours, len(pictures), what, channels) if colours is not None else None   # (before a device is looked at, too)
        tabs = _tone_arg(tones, len(pictures), what, channels) if tones is not None else None
    elif colours is not None or tones is not None:
        raise NhwError(f"{what}: `pictures` must be a list, one colour map or tone table a picture")
    table, _, dev = _picture_table(pictures, what, channels=channels)
    n = len(pictures)
    flags = _crop_flips(flips, n, what)
    out = torch.empty((n,) + fmt.shape(out_h, out_w), dtype=fmt.dtype, device=dev)
    addr = out.data_ptr() + torch.arange(n, dtype=torch.int64) * (channels * out_h * out_w * out.element_size())
    addr = addr.to(dev)
    d_flags = torch.from_numpy(flags).to(dev) if flags is not None else None
    L = _library()
    c = fmt.c_struct()
    d_maps = _device_table(maps, dev) if colours is not None else None
    d_tones = _device_tones(tabs, dev, what) if tones is not None else None
    call, tables = _sample_entry(L, "resample", channels, d_maps, d_tones)
    with torch.cuda.device(dev):
        rc = call(table.data_ptr(), n, out_w, out_h, RESAMPLERS[filter], ctypes.byref(c), d_flags.data_ptr() if d_flags is not None else None,
                  *(t.data_ptr() if t is not None else None for t in tables), addr.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


# ---------------------------------------------------------------- affine warps into tensors of one size
WARP_DTYPE = [("c", "<i8"), ("f", "<i8"), ("a", "<i4"), ("b", "<i4"), ("d", "<i4"), ("e", "<i4"), ("fill", "u1", (3,)), ("flags", "u1"), ("reserved", "<u4")]   # nhw_warp
WARP_MAX_STEP = 64                                 # NHW_WARP_MAX_STEP: a step of the grid is 64 source pixels an output pixel at the most
WARP_BORDERS = {"fill": 0, "replicate": 1}         # bit 0 of nhw_warp.flags: NHW_WARP_REPLICATE
_WARP_STEP, _WARP_OFFSET = WARP_MAX_STEP << 16, 1 << 40


def _warp_matrix(matrix, what):
    """`matrix` as a float64 array [2, 3] of finite numbers, or raises"""
    import numpy as np
    try:
        m = np.asarray(matrix)
        m = m.astype(np.float64) if m.dtype.kind in "iuf" else None
    except (TypeError, ValueError):
        m = None
    if m is None or m.shape != (2, 3):
        raise NhwError(f"{what}: a warp is a 2 x 3 matrix [[A, B, C], [D, E, F]] of numbers, got {matrix!r}")
    if not np.isfinite(m).all():
        raise NhwError(f"{what}: a warp's entries must be finite, got {m.tolist()!r}")
    return m


def _warp_within(six, what):
    """the six integers (a, b, c, d, e, f) of a warp inside nhw_warp's limits, or raises"""
    a, b, c, d, e, f = six
    if any(abs(v) > _WARP_STEP for v in (a, b, d, e)) or any(abs(v) > _WARP_OFFSET for v in (c, f)):
        raise NhwError(f"{what}: the warp {tuple(six)!r} is beyond the limits: steps of {WARP_MAX_STEP} source pixels an output pixel (2^22), offsets of 2^24 pixels (2^40)")
    return tuple(int(v) for v in six)


def warp_fixed(matrix):
    """A warp in nhw_warp's fixed point.  matrix: 2 x 3 floats [[A, B, C], [D, E, F]] that map the centre (ox + 1/2, oy + 1/2) of output pixel
    (ox, oy) to continuous source coordinates in which pixel i covers [i, i + 1): sx = A (ox + 1/2) + B (oy + 1/2) + C, sy alike -> the six
    integers (a, b, c, d, e, f) of DESIGN.md section 21: a = rint(65536 A), b, d, e alike, c = rint(65536 (C - 1/2)), f = rint(65536 (F - 1/2)),
    in float64, ties to even (the -1/2 moves to the grid on which pixel i has its centre at i).  Raises NhwError for an entry that is not
    finite or beyond the limits: |a|, |b|, |d|, |e| <= 2^22 (WARP_MAX_STEP pixels), |c|, |f| <= 2^40."""
    import numpy as np
    m = _warp_matrix(matrix, "warp_fixed")
    v = np.rint(np.array([m[0, 0], m[0, 1], m[0, 2] - 0.5, m[1, 0], m[1, 1], m[1, 2] - 0.5]) * 65536.0)
    if not (np.isfinite(v).all() and (np.abs(v[[0, 1, 3, 4]]) <= _WARP_STEP).all() and (np.abs(v[[2, 5]]) <= _WARP_OFFSET).all()):
        raise NhwError(f"warp_fixed: the warp {m.tolist()!r} is beyond the limits: steps of {WARP_MAX_STEP} source pixels an output pixel, offsets of 2^24 pixels")
    return tuple(int(x) for x in v)


def warp_scale(matrix) -> int:
    """the scale to decode at for a warp in full-resolution coordinates: the largest s of 4, 2 with min(hypot(A, D), hypot(B, E)) >= s, else
    1 -- the lengths of the steps along the two output axes, so that at that scale the two taps see a reduction below 2 along both (where
    the steps are below 8 pixels; beyond that the filter aliases as section 18's does)"""
    m = _warp_matrix(matrix, "warp_scale")
    n = min(math.hypot(m[0, 0], m[1, 0]), math.hypot(m[0, 1], m[1, 1]))
    return 4 if n >= 4 else 2 if n >= 2 else 1


def _warp_index(six, ox, oy):
    """(ix, iy) of output pixel (ox, oy) under section 21's rule, in Python's integers (>> floors)"""
    a, b, c, d, e, f = six
    sx, sy = ((a * (2 * ox + 1) + b * (2 * oy + 1)) >> 1) + c, ((d * (2 * ox + 1) + e * (2 * oy + 1)) >> 1) + f
    return (sx + 128) >> 16, (sy + 128) >> 16


def warp_window(matrix, size, pic_w: int, pic_h: int, scale: int) -> tuple:
    """The window of a pic_w x pic_h picture at `scale` that a warp needs, and the warp in that window's coordinates.  matrix: as for
    warp_fixed, in full-resolution coordinates; size = (out_h, out_w) -> ((x0, y0, w0, h0), fixed').  With m = warp_fixed(matrix / scale) the
    rule's own ix, iy at the four corner output pixels are the extremes (the position is monotone along either output axis); the window is
    min ix .. max ix + 1 by min iy .. max iy + 1, each bound clamped into the scaled picture (scaled_size), so it is never empty, holds every
    tap that lies in the picture and the clamp of every tap that does not; fixed' is m with c - 65536 x0 and f - 65536 y0, an exact
    translation, which never takes a warp out of the limits: x0 is above 0 only where some position is -- then c is above -2^36, the
    reach of 4096 steps of 64 pixels --, and it is below 2^16, so c - 65536 x0 lies between -2^36 - 2^32 and c.  The warp of the window under fixed' is therefore, byte for byte, the warp of the whole scaled picture under m, with
    either border."""
    what = "warp_window"
    scale = _scale(scale, what)
    out_h, out_w = _crop_size(size, what)
    sw, sh = scaled_size(pic_w, pic_h, scale)
    m = warp_fixed(_warp_matrix(matrix, what) / scale)
    at = [_warp_index(m, ox, oy) for ox in (0, out_w - 1) for oy in (0, out_h - 1)]
    clamp = lambda v, n: min(max(v, 0), n - 1)
    x0, x1 = clamp(min(p[0] for p in at), sw), clamp(max(p[0] for p in at) + 1, sw)
    y0, y1 = clamp(min(p[1] for p in at), sh), clamp(max(p[1] for p in at) + 1, sh)
    fixed = _warp_within((m[0], m[1], m[2] - 65536 * x0, m[3], m[4], m[5] - 65536 * y0), what)
    return (x0, y0, x1 - x0 + 1, y1 - y0 + 1), fixed


def crop_warp(x, y, w, h, size, angle=0.0, flip=False):
    """RandomResizedCrop + RandomRotation as one warp: the 2 x 3 matrix (numpy float64, as warp_fixed takes it) that lays the out_w x out_h
    output, size = (out_h, out_w), over the w x h rectangle at (x, y) of the source -- numbers, in the continuous coordinates of warp_fixed --,
    turned by `angle` radians about the rectangle's centre and mirrored left-right with `flip`.  With u = ((ox + 1/2) / out_w - 1/2) w (its
    sign changed by `flip`) and v = ((oy + 1/2) / out_h - 1/2) h, the source position is (x + w / 2 + u cos - v sin, y + h / 2 + u sin + v
    cos): angle 0 is the crop resized with two taps, a positive angle turns the sampling grid from the +x axis towards the +y axis of the
    source.  Coordinates and the sense of rotation are those of the STORED rows (row 0 is the first row of the byte picture): under
    rows="reversed" on a bottom-up file, where the tensor shows the picture upright, a positive angle appears to turn the other way."""
    import numpy as np
    what = "crop_warp"
    out_h, out_w = _crop_size(size, what)
    try:
        x, y, w, h, angle = (float(v) for v in (x, y, w, h, angle))
    except (TypeError, ValueError):
        raise NhwError(f"{what}: x, y, w, h and angle must be numbers") from None
    if not all(math.isfinite(v) for v in (x, y, w, h, angle)) or w <= 0 or h <= 0:
        raise NhwError(f"{what}: the rectangle {x!r}, {y!r}, {w!r} x {h!r} is empty or not finite, or the angle {angle!r} is not finite")
    cs, sn = math.cos(angle), math.sin(angle)
    ux, vy = (-w if flip else w) / out_w, h / out_h                      # u = ux (ox + 1/2) - (ux out_w) / 2, v = vy (oy + 1/2) - h / 2
    u0, v0 = -ux * out_w / 2, -h / 2
    return np.array([[cs * ux, -sn * vy, x + w / 2 + cs * u0 - sn * v0], [sn * ux, cs * vy, y + h / 2 + sn * u0 + cs * v0]], dtype=np.float64)


def _warp_border(fill, border, what, channels=3):
    """the checked (fill bytes B, G, R; flag byte) of a warp call; channels=1: fill is one byte, which goes into the first place"""
    if not isinstance(border, str) or border not in WARP_BORDERS:
        raise NhwError(f"{what}: `border` must be one of {', '.join(repr(k) for k in WARP_BORDERS)}, got {border!r}")
    if channels == 1:
        if isinstance(fill, bool) or not isinstance(fill, numbers.Integral) or not 0 <= fill <= 255:
            raise NhwError(f"{what}: `fill` must be one byte, an integer of 0 .. 255, got {fill!r}")
        return (int(fill), 0, 0), WARP_BORDERS[border]
    if not (isinstance(fill, (tuple, list)) and len(fill) == 3 and all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and 0 <= v <= 255 for v in fill)):
        raise NhwError(f"{what}: `fill` must be three bytes (B, G, R), got {fill!r}")
    return tuple(int(v) for v in fill), WARP_BORDERS[border]


def _warp_entry(matrix, what):
    """one entry of `matrices`: the six integers (a, b, c, d, e, f) as they are -- a flat sequence of six integers, or an array of an integer
    dtype, [6] or [2, 3] -- or a 2 x 3 matrix of floats, which goes through warp_fixed"""
    import numpy as np
    try:
        m = np.asarray(matrix)
    except Exception:
        m = None
    if m is not None and m.dtype.kind in "iu" and (m.shape == (6,) or (m.shape == (2, 3) and isinstance(matrix, np.ndarray))):
        return _warp_within([int(v) for v in m.reshape(6)], what)
    if m is None or m.shape != (2, 3) or m.dtype.kind not in "iuf":
        raise NhwError(f"{what}: a warp is a 2 x 3 matrix of floats or the six integers (a, b, c, d, e, f), got {matrix!r}")
    return warp_fixed(m)


def _warp_table(fixed, fill, flags):
    """the nhw_warp table of a list of six-integer warps, a numpy array of WARP_DTYPE"""
    import numpy as np
    t = np.zeros(len(fixed), WARP_DTYPE)
    for i, (a, b, c, d, e, f) in enumerate(fixed):
        t[i] = (c, f, a, b, d, e, fill, flags, 0)
    return t


def warp_to_tensor_device(pictures, matrices, size, fmt, fill=(0, 0, 0), border="fill", colours=None, tones=None):
    """Pictures sampled along tilted grids into one batch tensor of one size (k_warp_to_tensor, nhw_warp_to_tensor_device, DESIGN.md section
    21): pictures as for resize_to_tensor_device, matrices one warp a picture -- a 2 x 3 matrix of floats as warp_fixed takes it, in the
    picture's own coordinates, or the six integers (a, b, c, d, e, f) as warp_fixed returns them (a flat sequence of six integers, or an array
    of an integer dtype) --, size = (out_h, out_w) -> a new tensor [n, 3, out_h, out_w] or [n, out_h, out_w, 3] of fmt.dtype.  Two taps a
    direction at the position the warp gives, in integers; a tap outside the picture takes fill = (B, G, R), or with border="replicate" the
    nearest edge pixel.  Reads only the pictures' own bytes.  Ordered on torch's current stream.  colours: as for resize_to_tensor_device
    (nhw_warp_mapped_to_tensor_device); the border colour is mapped like any other pixel.  tones: as for resize_to_tensor_device
    (nhw_warp_toned_to_tensor_device); the border colour goes through the table too."""
    return _warp_to_tensor("warp_to_tensor_device", 3, pictures, matrices, size, fmt, fill, border, colours, tones)


def warp_grey_to_tensor_device(pictures, matrices, size, fmt, fill=0, border="fill", colours=None, tones=None):
    """warp_to_tensor_device for one-channel pictures (nhw_warp_grey_to_tensor_device): pictures and fmt as for
    resize_grey_to_tensor_device, fill one byte -> a new tensor [n, 1, out_h, out_w] or [n, out_h, out_w, 1] of fmt.dtype; colours and tones as there."""
    return _warp_to_tensor("warp_grey_to_tensor_device", 1, pictures, matrices, size, fmt, fill, border, colours, tones)


def _warp_to_tensor(what, channels, pictures, matrices, size, fmt, fill, border, colours=None, tones=None):
    """warp_to_tensor_device (channels=3) and warp_grey_to_tensor_device (1)"""
    import numpy as np
    import torch
    fmt = _tensor_format(fmt, what, grey=channels == 1)
    out_h, out_w = _crop_size(size, what)
    fill, flags = _warp_border(fill, border, what, channels)
    if not isinstance(pictures, (list, tuple)) or not isinstance(matrices, (list, tuple, np.ndarray)) or len(matrices) != len(pictures):
        raise NhwError(f"{what}: `pictures` and `matrices` must be lists of the same length, one warp a picture")
    warps = _warp_table([_warp_entry(m, f"{what}: matrix {i}") for i, m in enumerate(matrices)], fill, flags)
    maps = _colour_table(colours, len(pictures), what, channels) if colours is not None else None
    tabs = _tone_arg(tones, len(pictures), what, channels) if tones is not None else None
    table, _, dev = _picture_table(pictures, what, channels=channels)
    n = len(pictures)
    out = torch.empty((n,) + fmt.shape(out_h, out_w), dtype=fmt.dtype, device=dev)
    addr = out.data_ptr() + torch.arange(n, dtype=torch.int64) * (channels * out_h * out_w * out.element_size())
    addr = addr.to(dev)
    d_warps = torch.from_numpy(warps.view(np.int64).copy()).to(dev)
    L = _library()
    c = fmt.c_struct()
    d_maps = _device_table(maps, dev) if colours is not None else None
    d_tones = _device_tones(tabs, dev, what) if tones is not None else None
    call, tables = _sample_entry(L, "warp", channels, d_maps, d_tones)
    with torch.cuda.device(dev):
        rc = call(table.data_ptr(), n, out_w, out_h, ctypes.byref(c), d_warps.data_ptr(), *(t.data_ptr() if t is not None else None for t in tables), addr.data_ptr(),
                  torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


# ---------------------------------------------------------------- a colour matrix a sample
COLOUR_DTYPE = [("m", "<i4", (3, 3)), ("o", "<i4", (3,)), ("reserved", "<u4", (4,))]   # nhw_colour_map, 64 bytes
COLOUR_MAX_GAIN = 16                               # NHW_COLOUR_MAX_GAIN: a matrix entry is 16 in magnitude at the most (2^20 / 65536)
COLOUR_MAX_OFFSET = 4096                           # NHW_COLOUR_MAX_OFFSET: an offset is 4096 grey levels in magnitude at the most (2^28 / 65536)
_COLOUR_GAIN, _COLOUR_OFFSET = COLOUR_MAX_GAIN << 16, COLOUR_MAX_OFFSET << 16
_YIQ = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.322), (0.211, -0.523, 0.312))


def _colour_affine(matrix, what):
    """`matrix` as a float64 array [3, 4] of finite numbers, or raises"""
    import numpy as np
    try:
        m = np.asarray(matrix)
        m = m.astype(np.float64) if m.dtype.kind in "iuf" else None
    except (TypeError, ValueError):
        m = None
    if m is None or m.shape != (3, 4):
        raise NhwError(f"{what}: a colour map is a 3 x 4 matrix of numbers on (R, G, B, 1), got {matrix!r}")
    if not np.isfinite(m).all():
        raise NhwError(f"{what}: a colour map's entries must be finite, got {m.tolist()!r}")
    return m


def colour_compose(first, then):
    """the affine map that applies `first` and then `then`, both float [3, 4] on (R, G, B, 1): then[:, :3] @ first, with then's offset added"""
    import numpy as np
    a, b = _colour_affine(first, "colour_compose"), _colour_affine(then, "colour_compose")
    return np.concatenate([b[:, :3] @ a[:, :3], (b[:, :3] @ a[:, 3] + b[:, 3])[:, None]], axis=1)


def colour_matrix(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, centre=128.0):
    """ColorJitter as one affine map: a float64 [3, 4] matrix on (R, G, B, 1) in byte units (0 .. 255), the composition, applied in this order,
    of brightness x -> b x; contrast x -> c x + (1 - c) centre; saturation x -> s x + (1 - s) L with L = 0.299 R + 0.587 G + 0.114 B; and hue,
    a rotation by 2 pi hue of the I, Q plane of YIQ, inv(T) Rot T with T = [[0.299, 0.587, 0.114], [0.596, -0.274, -0.322], [0.211, -0.523,
    0.312]] -- the linear form DALI and TensorFlow use, which keeps Y and keeps greys grey.  colour_fixed turns it into the integers the mapped
    calls take; colour_compose chains it with other maps (a channel mix, an inversion, a grey).
    This is not torchvision's chain, bit for bit or otherwise: there is no clamp to 0 .. 255 between the steps (only the one at the end of the
    rule), contrast pivots on the given `centre`, not on the picture's own mean grey, and hue is the linear YIQ turn, not a shift of H through
    HSV."""
    import numpy as np
    try:
        b, c, s, h, z = (float(v) for v in (brightness, contrast, saturation, hue, centre))
    except (TypeError, ValueError):
        raise NhwError("colour_matrix: brightness, contrast, saturation, hue and centre must be numbers") from None
    if not all(math.isfinite(v) for v in (b, c, s, h, z)):
        raise NhwError(f"colour_matrix: the parameters must be finite, got {(brightness, contrast, saturation, hue, centre)!r}")
    eye, zero = np.eye(3), np.zeros((3, 1))
    luma = np.tile(np.array(_YIQ[0]), (3, 1))
    t = np.array(_YIQ)
    cs, sn = math.cos(2 * math.pi * h), math.sin(2 * math.pi * h)
    rot = np.array([[1.0, 0.0, 0.0], [0.0, cs, -sn], [0.0, sn, cs]])
    steps = [np.hstack([b * eye, zero]), np.hstack([c * eye, np.full((3, 1), (1 - c) * z)]), np.hstack([s * eye + (1 - s) * luma, zero]),
             np.hstack([np.linalg.solve(t, rot @ t) if h else eye, zero])]     # (no turn is the identity exactly, not to the solver's last bit)
    m = steps[0]
    for step in steps[1:]:
        m = colour_compose(m, step)
    return m


def colour_fixed(matrix):
    """A colour map in nhw_colour_map's fixed point.  matrix: 3 x 4 floats on (R, G, B, 1) in byte units, as colour_matrix returns it -> the twelve
    integers of the struct in its order B, G, R: m[0][0], m[0][1], .. m[2][2], then o[0], o[1], o[2], each rint(65536 value) in float64, ties to
    even, with rows and columns 0 and 2 of the matrix exchanged (row 0 of the struct makes B, column 0 reads B).  Raises NhwError for an entry
    that is not finite or beyond the limits: |m| <= 2^20 (COLOUR_MAX_GAIN), |o| <= 2^28 (COLOUR_MAX_OFFSET grey levels)."""
    import numpy as np
    a = _colour_affine(matrix, "colour_fixed")
    v = np.rint(a[::-1] * 65536.0)
    m, o = v[:, 2::-1], v[:, 3]
    if not ((np.abs(m) <= _COLOUR_GAIN).all() and (np.abs(o) <= _COLOUR_OFFSET).all()):
        raise NhwError(f"colour_fixed: the map {a.tolist()!r} is beyond the limits: matrix entries of {COLOUR_MAX_GAIN}, offsets of {COLOUR_MAX_OFFSET} grey levels")
    return tuple(int(x) for x in m.reshape(9)) + tuple(int(x) for x in o)


def _colour_table(colours, n, what, channels=3):
    """the nhw_colour_map table of a call's `colours`, a numpy array of COLOUR_DTYPE: n entries, each a 3 x 4 matrix of floats (through
    colour_fixed) or the twelve integers as colour_fixed returns them (an integer array [12]); channels=1: each a pair (gain, offset), which
    goes to m[0][0] and o[0] as rint(65536 value).  Host only; raises for a wrong count or shape, a number that is not finite, a map beyond
    the limits"""
    import numpy as np
    if not isinstance(colours, (list, tuple, np.ndarray)) or len(colours) != n:
        raise NhwError(f"{what}: `colours` must be {n} colour maps, one a sample, got {len(colours) if hasattr(colours, '__len__') else colours!r}")
    t = np.zeros(n, COLOUR_DTYPE)
    for i, c in enumerate(colours):
        who = f"{what}: colours[{i}]"
        try:
            a = np.asarray(c)
        except Exception:
            a = None
        if channels == 1:
            if a is None or a.shape != (2,) or a.dtype.kind not in "iuf":
                raise NhwError(f"{who}: a grey call takes a pair (gain, offset) of numbers, got {c!r}")
            a = a.astype(np.float64)
            v = np.rint(a * 65536.0)
            if not np.isfinite(a).all() or abs(v[0]) > _COLOUR_GAIN or abs(v[1]) > _COLOUR_OFFSET:
                raise NhwError(f"{who}: the pair {a.tolist()!r} is not finite or beyond the limits: a gain of {COLOUR_MAX_GAIN}, an offset of {COLOUR_MAX_OFFSET} grey levels")
            t[i]["m"][0, 0], t[i]["o"][0] = int(v[0]), int(v[1])
            continue
        if a is not None and a.dtype.kind in "iu" and a.shape == (12,):
            twelve = [int(x) for x in a]
            if any(abs(x) > _COLOUR_GAIN for x in twelve[:9]) or any(abs(x) > _COLOUR_OFFSET for x in twelve[9:]):
                raise NhwError(f"{who}: the map {tuple(twelve)!r} is beyond the limits: matrix entries of 2^20, offsets of 2^28")
        else:
            try:
                twelve = colour_fixed(_colour_affine(c, who))
            except NhwError as e:
                raise NhwError(f"{who}: {e}") from None
        t[i]["m"], t[i]["o"] = np.array(twelve[:9]).reshape(3, 3), twelve[9:]
    return t


def _device_table(maps, dev):
    """a table of COLOUR_DTYPE on the device, as 64-bit words"""
    import numpy as np
    import torch
    return torch.from_numpy(np.ascontiguousarray(maps).view(np.int64).copy()).to(dev)


# ---------------------------------------------------------------- a tone table a sample; histograms
TONE_OPS = {"keep": 0, "equalize": 1, "autocontrast": 2}     # NHW_TONE_KEEP, NHW_TONE_EQUALIZE, NHW_TONE_AUTOCONTRAST


def _tone_values(v, what, name, lo, hi, integral=False):
    """one number, or three for the channels R, G, B -> three floats (ints with `integral`) in lo .. hi, or raises"""
    import numpy as np
    vs = list(v) if isinstance(v, (list, tuple)) or (isinstance(v, np.ndarray) and v.ndim == 1) else [v] * 3
    if len(vs) != 3:
        raise NhwError(f"{what}: {name} is one value or three, one a channel, got {v!r}")
    out = []
    for x in vs:
        ok = not isinstance(x, bool) and isinstance(x, numbers.Integral if integral else numbers.Real)
        if ok and not integral:
            ok = math.isfinite(x)
        if not ok or not lo <= x <= hi:
            raise NhwError(f"{what}: {name} must be {'an integer' if integral else 'a finite number'} of {lo} .. {hi}, got {x!r}")
        out.append(int(x) if integral else float(x))
    return out


def _tone_check(table, what, channels=3):
    """`table` as a uint8 array [3, 256] (channels=1: [256]) or raises: integers of 0 .. 255 in that shape"""
    import numpy as np
    try:
        a = np.asarray(table)
    except Exception:
        a = None
    shape = (3, 256) if channels == 3 else (256,)
    if a is None or a.dtype.kind not in "iu" or a.shape != shape or (a < 0).any() or (a > 255).any():
        raise NhwError(f"{what}: a tone table is {'3 x 256' if channels == 3 else '256'} integers of 0 .. 255, got {'an array of shape ' + str(a.shape) + ', ' + str(a.dtype) if a is not None and a.dtype.kind in 'iufb' else repr(table)}")
    return a.astype(np.uint8)


def tone_identity():
    """the tone table that changes nothing: uint8 [3, 256], row c the bytes 0 .. 255.  A tone table is what a pointwise
    operation on bytes is: row c (R, G, B) maps a byte of channel c; the toned calls apply it behind the blend and the colour map, in front of
    the value rule."""
    import numpy as np
    return np.tile(np.arange(256, dtype=np.uint8), (3, 1))


def tone_posterize(bits):
    """Posterize: x & ~(2^(8 - bits) - 1), the top `bits` bits kept; bits 0 .. 8, one value or three (R, G, B) -> uint8 [3, 256]"""
    import numpy as np
    x = np.arange(256)
    return np.stack([x & ~((1 << (8 - b)) - 1) & 255 for b in _tone_values(bits, "tone_posterize", "bits", 0, 8, integral=True)]).astype(np.uint8)


def tone_solarize(threshold):
    """Solarize: x where x < threshold, else 255 - x; threshold 0 .. 256 (0: the inversion, 256: the identity), one value or three -> uint8 [3, 256]"""
    import numpy as np
    x = np.arange(256)
    return np.stack([np.where(x < t, x, 255 - x) for t in _tone_values(threshold, "tone_solarize", "threshold", 0, 256)]).astype(np.uint8)


def tone_gamma(gamma, gain=1.0):
    """Gamma: rint(255 min(1, gain (x / 255)^gamma)) in float64, ties to even; gamma and gain of 0 .. 1000, each one value or three -> uint8
    [3, 256].  torchvision's adjust_gamma truncates where this rounds: its entries are this table's or one below."""
    import numpy as np
    x = np.arange(256) / 255.0
    gs, ks = _tone_values(gamma, "tone_gamma", "gamma", 0, 1000), _tone_values(gain, "tone_gamma", "gain", 0, 1000)
    return np.stack([np.rint(255.0 * np.minimum(1.0, k * x ** g)) for g, k in zip(gs, ks)]).astype(np.uint8)


def tone_affine(gain, offset):
    """The affine step a channel that must come AFTER a table, and so cannot be the colour matrix: clamp(floor(gain x + offset + 1/2), 0, 255),
    halves up at either sign; gain and offset finite and of -65536 .. 65536, each one value or three -> uint8 [3, 256]"""
    import numpy as np
    x = np.arange(256, dtype=np.float64)
    gs, os_ = _tone_values(gain, "tone_affine", "gain", -65536, 65536), _tone_values(offset, "tone_affine", "offset", -65536, 65536)
    return np.stack([np.clip(np.floor(g * x + o + 0.5), 0, 255) for g, o in zip(gs, os_)]).astype(np.uint8)


def tone_compose(first, then):
    """the table that applies `first` and then `then`: row c is then[c][first[c][x]]"""
    import numpy as np
    a, b = _tone_check(first, "tone_compose"), _tone_check(then, "tone_compose")
    return np.stack([b[c][a[c]] for c in range(3)])


def tone_fixed(table):
    """a tone table in nhw_tone_table's layout: uint8 [3, 256] on R, G, B -> the struct's 768 bytes, rows in its order B, G, R"""
    import numpy as np
    return np.ascontiguousarray(_tone_check(table, "tone_fixed")[::-1]).reshape(768)


def _tone_arg(tones, n, what, channels=3):
    """a call's `tones`: a uint8 CUDA tensor [n, 768] already in the struct's order (returned as it is), or n tables -- [3, 256] on R, G, B,
    channels=1: [256], which goes to t[0] -- as a numpy uint8 array [n, 768].  No device is touched; raises for a wrong count, shape or value"""
    import numpy as np
    if hasattr(tones, "is_cuda"):
        if not tones.is_cuda or str(tones.dtype) != "torch.uint8" or tuple(tones.shape) != (n, 768) or not tones.is_contiguous():
            raise NhwError(f"{what}: `tones` as a tensor must be a contiguous uint8 CUDA tensor [{n}, 768], got {tuple(tones.shape)} {tones.dtype} on {tones.device}")
        return tones
    if not isinstance(tones, (list, tuple, np.ndarray)) or len(tones) != n:
        raise NhwError(f"{what}: `tones` must be {n} tone tables, one a sample, got {len(tones) if hasattr(tones, '__len__') else tones!r}")
    t = np.zeros((n, 768), np.uint8)
    for i, x in enumerate(tones):
        a = _tone_check(x, f"{what}: tones[{i}]", channels)
        if channels == 3:
            t[i] = a[::-1].reshape(768)
        else:
            t[i, :256] = a
    return t


def _decode_ops(n, flips, colours, tones, what, channels=3):
    """the per-sample tables of a full-file decode of n files, checked on the host before anything is launched ->
    (flags, maps, tones): the flag bytes as _crop_flips makes them, the nhw_colour_map table as _colour_table does, the tone tables as
    _tone_arg does (a CUDA tensor [n, 768] is passed on), each None where the argument is.  colours may be ONE map for all files -- a 3 x 4
    matrix, the twelve integers of colour_fixed, for grey one pair (gain, offset) -- or n of them."""
    import numpy as np
    flags = _crop_flips(flips, n, what)
    maps = None
    if colours is not None:
        try:
            a = np.asarray(colours)
        except Exception:
            a = None
        one = a is not None and a.dtype.kind in "iuf" and (a.shape == (2,) if channels == 1 else a.shape == (3, 4) or (a.shape == (12,) and a.dtype.kind in "iu"))
        maps = _colour_table([colours] * n if one else colours, n, what, channels)
    return flags, maps, _tone_arg(tones, n, what, channels) if tones is not None else None


def _host_tones(tones, n, what, channels=3):
    """_tone_arg for the decoder's calls, whose tables are read from host memory: a tensor is no table here"""
    if hasattr(tones, "is_cuda"):
        raise NhwError(f"{what}: `tones` must be {n} tone tables in host memory, one a sample, not a tensor")
    return _tone_arg(tones, n, what, channels)


def _device_tones(tabs, dev, what):
    """_tone_arg's result on the device `dev`"""
    import torch
    if isinstance(tabs, torch.Tensor):
        if tabs.device != dev:
            raise NhwError(f"{what}: `tones` is on {tabs.device}, the pictures on {dev}")
        return tabs
    return torch.from_numpy(tabs).to(dev)


def hist_device(pictures):
    """The byte histograms of pictures (k_hist_bytes, nhw_hist_device): a list of uint8 CUDA tensors, all [H, W, 3] as
    resize_to_tensor_device takes them or all [H, W] as resize_grey_to_tensor_device does -> an int64 CUDA tensor [n, C, 256], C = 3 or 1:
    entry [k, c, v] is the number of pixels of picture k whose byte c is v (c in the pictures' own order, B, G, R for the byte path's).  Reads
    only the pictures' own bytes; integer sums, the same result every run.  Ordered on torch's current stream."""
    import torch
    what = "hist_device"
    channels = 1 if isinstance(pictures, (list, tuple)) and pictures and len(getattr(pictures[0], "shape", ())) == 2 else 3
    table, _, dev = _picture_table(pictures, what, channels=channels)
    n = len(pictures)
    hist = torch.empty((n, channels, 256), dtype=torch.int32, device=dev)
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_hist_device(table.data_ptr(), n, channels, hist.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return hist.to(torch.int64) & 0xFFFFFFFF


def tone_from_hist_device(hist_u32, ops, tones=None):
    """Tone tables from histograms on the device (k_tone_from_hist, nhw_tone_from_hist_device).  hist_u32: a CUDA tensor
    [n, C, 256], C = 3 or 1, int64 as hist_device returns it (counts of 0 .. 2^32 - 1) or int32 holding the uint32 words; ops: one of "keep",
    "equalize", "autocontrast" a sample; tones: the tables whose rows "keep" keeps -- as the toned calls take them, n tables [3, 256] (C = 1:
    [256]) or a uint8 CUDA tensor [n, 768] --, the identity by default -> a new uint8 CUDA tensor [n, 768] in nhw_tone_table's order, row c made
    from histogram c, which the toned calls take as `tones`.  "equalize" is PIL's ImageOps.equalize and torchvision's equalize; "autocontrast" is
    torchvision's rule in exact integers (torchvision computes in float32 and may differ by one level).  With C = 1 only the first 256 bytes of
    a table are written.  Ordered on torch's current stream.
    The Equalize recipe, crops to an equalized training batch without leaving the device:
      1. batch, _ = decoder.decode_crops_device(containers, crops, (224, 224), TensorFormat("uint8", "HWC", "BGR", "file"));
      2. hist = hist_device(list(batch));                                  (the views batch[k], [224, 224, 3])
      3. tables = tone_from_hist_device(hist, ["equalize"] * len(batch));
      4. out = resize_to_tensor_device(list(batch), (224, 224), final_format, tones=tables)
    -- the resample of a picture to its own size is the identity, so step 4 is the table and the value rule."""
    import numpy as np
    import torch
    what = "tone_from_hist_device"
    if not (isinstance(hist_u32, torch.Tensor) and hist_u32.is_cuda and hist_u32.dtype in (torch.int64, torch.int32) and hist_u32.dim() == 3
            and hist_u32.shape[0] >= 1 and hist_u32.shape[1] in (1, 3) and hist_u32.shape[2] == 256):
        raise NhwError(f"{what}: the histograms must be an int64 or int32 CUDA tensor [n, 3 or 1, 256]")
    n, channels, dev = int(hist_u32.shape[0]), int(hist_u32.shape[1]), hist_u32.device
    if not isinstance(ops, (list, tuple)) or len(ops) != n or any(not isinstance(o, str) or o not in TONE_OPS for o in ops):
        raise NhwError(f"{what}: `ops` must be {n} of {sorted(TONE_OPS)}, one a sample")
    tabs = _tone_arg(tones, n, what, channels) if tones is not None else np.tile(tone_fixed(tone_identity()), (n, 1))
    d_tones = _device_tones(tabs, dev, what).clone()
    h = hist_u32
    if h.dtype == torch.int64:
        h = torch.where(h >= 2 ** 31, h - 2 ** 32, h).to(torch.int32)
    h = h.contiguous()
    d_ops = torch.tensor([TONE_OPS[o] for o in ops], dtype=torch.uint8).to(dev)
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_tone_from_hist_device(h.data_ptr(), n, channels, d_ops.data_ptr(), d_tones.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return d_tones


# ---------------------------------------------------------------- blur and sharpen a sample
BLUR_DTYPE = [("wx", "<u2", (32,)), ("wy", "<u2", (32,)), ("mix", "<i4"), ("rx", "u1"), ("ry", "u1"), ("border", "u1"), ("reserved8", "u1"), ("reserved", "<u4", (2,))]   # nhw_blur, 144 bytes
BLUR_MAX_RADIUS = 15                               # NHW_BLUR_MAX_RADIUS: 31 taps a direction at the most
BLUR_ONE = 32768                                   # NHW_BLUR_ONE: a tap is in 1/32768, and a direction's taps sum to this
BLUR_MAX_MIX = 16                                  # NHW_BLUR_MAX_MIX: |mix| is 16 at the most (2^20 / 65536)
BLUR_BORDERS = {"reflect": 0, "replicate": 1}      # NHW_BLUR_REFLECT, NHW_BLUR_REPLICATE


def blur_taps(weights):
    """The integer taps of a list of weights: any non-negative finite floats, of odd length 31 at the most and not all zero -> a tuple of ints
    summing to exactly BLUR_ONE.  The weights are normalised in float64, each becomes rint(32768 w), and what the sum then lacks or exceeds
    goes to the centre tap; raises NhwError where that would make the centre tap negative."""
    import numpy as np
    try:
        w = np.asarray(weights)
        w = w.astype(np.float64) if w.dtype.kind in "iuf" else None
    except (TypeError, ValueError):
        w = None
    if w is None or w.ndim != 1 or len(w) % 2 != 1 or len(w) > 2 * BLUR_MAX_RADIUS + 1:
        raise NhwError(f"blur_taps: the weights are a list of numbers of odd length {2 * BLUR_MAX_RADIUS + 1} at the most, got {weights!r}")
    if not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0 or not np.isfinite(w.sum()):
        raise NhwError(f"blur_taps: the weights must be finite, none below zero and not all zero, got {w.tolist()!r}")
    t = np.rint(BLUR_ONE * (w / w.sum())).astype(np.int64)
    t[len(t) // 2] += BLUR_ONE - int(t.sum())
    if t[len(t) // 2] < 0:
        raise NhwError(f"blur_taps: the roundings of {w.tolist()!r} leave the centre tap below zero")
    return tuple(int(v) for v in t)


def _blur_radius(radius, what):
    if isinstance(radius, bool) or not isinstance(radius, numbers.Integral) or not 0 <= radius <= BLUR_MAX_RADIUS:
        raise NhwError(f"{what}: the radius must be an integer of 0 .. {BLUR_MAX_RADIUS}, got {radius!r}")
    return int(radius)


def blur_gaussian(sigma, radius=None):
    """torchvision's gaussian_blur weights as taps: exp(-1/2 (x / sigma)^2) on x = -radius .. radius, through blur_taps.  sigma: a finite number
    above 0; radius: 0 .. BLUR_MAX_RADIUS, or None for min(15, ceil(3 sigma)) and 1 at the least.  (torchvision's kernel_size is 2 radius + 1.)"""
    import numpy as np
    if isinstance(sigma, bool) or not isinstance(sigma, numbers.Real) or not math.isfinite(sigma) or not sigma > 0:
        raise NhwError(f"blur_gaussian: sigma must be a finite number above 0, got {sigma!r}")
    r = max(1, min(BLUR_MAX_RADIUS, math.ceil(3 * float(sigma)))) if radius is None else _blur_radius(radius, "blur_gaussian")
    x = np.arange(-r, r + 1, dtype=np.float64)
    return blur_taps(np.exp(-0.5 * (x / float(sigma)) ** 2))


def blur_box(radius):
    """the box filter of 2 radius + 1 equal weights, through blur_taps"""
    return blur_taps([1.0] * (2 * _blur_radius(radius, "blur_box") + 1))


def _blur_tap_list(taps, what):
    """a tap list of blur_fixed: integers that already sum to BLUR_ONE are taken as they are, anything else goes through blur_taps"""
    import numpy as np
    try:
        a = np.asarray(taps)
    except Exception:
        a = None
    if a is not None and a.ndim == 1 and a.dtype.kind in "iu" and len(a) % 2 == 1 and len(a) <= 2 * BLUR_MAX_RADIUS + 1 and (a >= 0).all() and int(a.sum()) == BLUR_ONE:
        return tuple(int(v) for v in a)
    try:
        return blur_taps(taps)
    except NhwError as e:
        raise NhwError(f"{what}: {e}") from None


def blur_fixed(taps_x, taps_y=None, mix=1.0, border="reflect"):
    """One nhw_blur record (a numpy scalar of BLUR_DTYPE), the separable filter of a sample under the rule of DESIGN.md section 26 -- rows, then
    columns, then the mix with the picture's own byte.  The rule and the record are what this build has; no device call applies a record yet.
    taps_x, taps_y: weights as blur_taps takes them, or integers that already sum to BLUR_ONE (what blur_gaussian and blur_box return); taps_y=None
    means taps_x.  mix: 1 the blurred pixel, 0 the picture's own, below 0 a sharpening (z = p + mix (b - p)); rint(65536 mix) in float64, ties to
    even, |mix| <= BLUR_MAX_MIX.  border: "reflect" (torch's reflect padding, torchvision's gaussian_blur) or "replicate".  Raises NhwError for a
    number that is not finite or beyond a limit.
    GaussianBlur(kernel_size=23, sigma=s) is blur_fixed(blur_gaussian(s, 11)); RandAugment's Sharpness of factor f is blur_fixed([1, 1, 1],
    mix=1 - f) up to PIL's non-separable 3 x 3 SMOOTH kernel, which this rule does not have."""
    import numpy as np
    wx = _blur_tap_list(taps_x, "blur_fixed: taps_x")
    wy = wx if taps_y is None else _blur_tap_list(taps_y, "blur_fixed: taps_y")
    if isinstance(mix, bool) or not isinstance(mix, numbers.Real) or not math.isfinite(mix):
        raise NhwError(f"blur_fixed: mix must be a finite number, got {mix!r}")
    m = float(np.rint(float(mix) * 65536.0))
    if abs(m) > BLUR_MAX_MIX * 65536:
        raise NhwError(f"blur_fixed: mix {mix!r} is beyond the limit of {BLUR_MAX_MIX} in magnitude")
    if not isinstance(border, str) or border not in BLUR_BORDERS:
        raise NhwError(f"blur_fixed: border must be one of {sorted(BLUR_BORDERS)}, got {border!r}")
    rec = np.zeros((), BLUR_DTYPE)
    rec["wx"][:len(wx)], rec["wy"][:len(wy)] = wx, wy
    rec["mix"], rec["rx"], rec["ry"], rec["border"] = int(m), len(wx) // 2, len(wy) // 2, BLUR_BORDERS[border]
    return rec[()]


TENSOR_PICTURE_DTYPE = [("addr", "<u8"), ("pitch", "<u8"), ("plane", "<u8"), ("width", "<u4"), ("height", "<u4"), ("first_tile", "<u4"), ("reserved", "<u4")]   # nhw_tensor_picture


def _tensor_batch(x, fmt, what, device=None):
    """x: a contiguous, 16-byte aligned CUDA tensor [n, 3, 512, 512] or [n, 512, 512, 3] of fmt.dtype (on cuda:device, if given) -> n"""
    import torch
    shape = fmt.shape(512, 512)
    if not (isinstance(x, torch.Tensor) and x.dim() == 4 and tuple(x.shape[1:]) == shape and x.shape[0] >= 1):
        raise NhwError(f"{what} wants a tensor of shape [n, {', '.join(map(str, shape))}] for {fmt.layout}, got {tuple(x.shape) if isinstance(x, torch.Tensor) else type(x).__name__}")
    if x.dtype != fmt.dtype:
        raise NhwError(f"{what}: the batch is {x.dtype}, the format {fmt.dtype}")
    if not x.is_cuda or (device is not None and x.device.index != device):
        raise NhwError(f"{what}: the batch is on {x.device}, not on " + ("a GPU" if device is None else f"cuda:{device}"))
    if not x.is_contiguous() or x.data_ptr() % 16:
        raise NhwError(f"{what}: the batch must be contiguous and 16-byte aligned")
    return int(x.shape[0])


def tensor_to_bytes_device(x, fmt):
    """The pictures the encoder makes of a tensor batch (k_tensor_to_bytes, nhw_tensor_to_bytes_device): x, a contiguous
    CUDA tensor [n, 3, 512, 512] (fmt.layout "CHW") or [n, 512, 512, 3] of fmt.dtype, read under fmt -> uint8 [n, 512, 512, 3] as encode_device
    and the fit searches take them.  The byte of element x of tensor channel c is rint(fmaf(float32(x), scale[c], bias[c])), ties to even,
    clamped to 0 .. 255, 0 for a NaN; uint8 passes the bytes on.  Ordered on torch's current stream."""
    import torch
    what = "tensor_to_bytes_device"
    fmt = _tensor_format(fmt, what)
    n = _tensor_batch(x, fmt, what)
    out = torch.empty((n, 512, 512, 3), dtype=torch.uint8, device=x.device)
    L = _library()
    c = fmt.c_struct()
    with torch.cuda.device(x.device):
        rc = L.nhw_tensor_to_bytes_device(x.data_ptr(), n, ctypes.byref(c), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def tensor_to_grey_bytes_device(x, fmt):
    """tensor_to_bytes_device for one-channel tensors (nhw_tensor_to_bytes_grey_device): x, a contiguous CUDA tensor
    [n, 1, 512, 512] or [n, 512, 512, 1] of fmt.dtype, fmt of channels "GREY" -> uint8 [n, 512, 512] as Encoder.encode_grey_device takes them, under
    the same value rule with the format's one scale and bias.  Ordered on torch's current stream."""
    import torch
    what = "tensor_to_grey_bytes_device"
    fmt = _tensor_format(fmt, what, grey=True)
    n = _tensor_batch(x, fmt, what)
    out = torch.empty((n, 512, 512), dtype=torch.uint8, device=x.device)
    L = _library()
    c = fmt.c_struct()
    with torch.cuda.device(x.device):
        rc = L.nhw_tensor_to_bytes_grey_device(x.data_ptr(), n, ctypes.byref(c), out.data_ptr(), torch.cuda.current_stream(x.device).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def _tensor_picture_table(tensors, fmt, what):
    """the checked nhw_tensor_picture table of a list of CUDA tensors [3, H, W] (strides (plane, pitch, 1)) or [H, W, 3] (strides (pitch, 3, 1))
    of fmt.dtype on one device -> (table as an int64 CUDA tensor, total tiles, device)"""
    import numpy as np
    import torch
    chw = fmt.layout == "CHW"
    form = "[3, H, W]" if chw else "[H, W, 3]"
    if not isinstance(tensors, (list, tuple)) or not tensors:
        raise NhwError(f"{what} wants a non-empty list of {fmt.dtype_name} CUDA tensors {form}")
    dev = tensors[0].device if isinstance(tensors[0], torch.Tensor) else None
    table = np.zeros(len(tensors), TENSOR_PICTURE_DTYPE)
    es = fmt.dtype.itemsize
    tiles = 0
    for i, x in enumerate(tensors):
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == fmt.dtype and x.dim() == 3 and x.shape[0 if chw else 2] == 3):
            raise NhwError(f"{what}: picture {i} is not a {fmt.dtype_name} CUDA tensor {form}")
        if x.device != dev:
            raise NhwError(f"{what}: picture {i} is on {x.device}, picture 0 on {dev}")
        h, w = (int(x.shape[1]), int(x.shape[2])) if chw else (int(x.shape[0]), int(x.shape[1]))
        t = picture_tiles(w, h)
        if chw:
            ok = (w == 1 or x.stride(2) == 1) and (h == 1 or x.stride(1) >= w) and x.stride(0) >= 0
            pitch, plane = (x.stride(1) if h > 1 else w) * es, x.stride(0) * es
        else:
            ok = x.stride(2) == 1 and (w == 1 or x.stride(1) == 3) and (h == 1 or x.stride(0) >= 3 * w)
            pitch, plane = (x.stride(0) if h > 1 else 3 * w) * es, 0
        if not ok:
            raise NhwError(f"{what}: picture {i} must have strides " + ("(plane, pitch >= W, 1)" if chw else "(pitch >= 3 W, 3, 1)") + f", got {tuple(x.stride())}")
        table[i] = (x.data_ptr(), pitch, plane, w, h, tiles, 0)
        tiles += t
    return torch.from_numpy(table.view(np.int64).copy()).to(dev), tiles, dev


def tile_tensors_device(tensors, fmt):
    """tile_pictures_device for tensor pictures (k_tile_pad_tensor, nhw_tile_tensors_device): a list of CUDA tensors of
    fmt.dtype on one device, [3, H, W] with element stride 1 along W (any row and plane stride: x[:, y0:y1, x0:x1] of a larger tensor works
    without a copy) or [H, W, 3] with strides (pitch, 3, 1), any H and W up to 65535 -> tiles uint8 [T, 512, 512, 3] of the byte pictures
    tensor_to_bytes_device's rule makes of them, padded by edge replication, picture after picture.  Reads only the pictures' own elements.
    Ordered on torch's current stream; feeds Encoder.encode_device and encode_fit_device."""
    import torch
    what = "tile_tensors_device"
    fmt = _tensor_format(fmt, what)
    table, tiles, dev = _tensor_picture_table(tensors, fmt, what)
    out = torch.empty((tiles, 512, 512, 3), dtype=torch.uint8, device=dev)
    L = _library()
    c = fmt.c_struct()
    with torch.cuda.device(dev):
        rc = L.nhw_tile_tensors_device(table.data_ptr(), len(tensors), 0, tiles, ctypes.byref(c), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def sse_pictures_device(tiles, pictures):
    """The exact SSE of decoded tiles against the pictures' own bytes (k_sse_crop, nhw_sse_pictures_device): tiles and pictures as for
    untile_pictures_device -> int64 tensor [n] on their device, zeroed and filled on torch's current stream.  The padding never counts:
    entry k equals the SSE between untile_pictures_device(tiles) and picture k."""
    import torch
    table, n_tiles, dev = _picture_tiles_arg(tiles, pictures, "sse_pictures_device")
    out = torch.zeros(len(pictures), dtype=torch.int64, device=dev)
    L = _library()
    with torch.cuda.device(dev):
        rc = L.nhw_sse_pictures_device(tiles.data_ptr(), table.data_ptr(), len(pictures), 0, n_tiles, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc != 0:
        raise NhwError(f"libnhwhip rc={rc}: {L.nhw_last_error().decode()}")
    return out


def picture_psnr_to_max_sse(db, width, height):
    """psnr_to_max_sse for a width x height picture: the largest SSE over its 3 W H bytes whose PSNR is at least `db`,
    floor(65025 * 3 W H * 10**(-db/10)) in float64 (exact: 65025 * 3 * 65535**2 < 2**53), for finite db > 0 and sides 1..65535.
    A number gives an int, an array (or list) of them an int64 numpy array.  For 512 x 512 it is psnr_to_max_sse(db)."""
    import numpy as np
    try:
        a = np.asarray(db, dtype=np.float64)
    except (TypeError, ValueError):
        raise NhwError(f"a PSNR target must be a finite number of dB above 0, got {db!r}") from None
    if a.size == 0 or not np.all(np.isfinite(a)) or not np.all(a > 0):
        raise NhwError(f"a PSNR target must be a finite number of dB above 0, got {db!r}")
    if not (isinstance(width, numbers.Integral) and isinstance(height, numbers.Integral)):
        raise NhwError(f"a picture's sides must be integers, got {width!r} x {height!r}")
    picture_tiles(int(width), int(height))
    m = np.floor(float(65025 * 3 * int(width) * int(height)) * np.power(10.0, -a / 10.0)).astype(np.int64)
    return int(m) if m.ndim == 0 else m


def picture_info(container) -> tuple:
    """(W, H) of a well-formed .nhwp container (nhw_picture_info); raises NhwError otherwise"""
    import numpy as np
    b = np.frombuffer(bytes(container), np.uint8)
    w, h = ctypes.c_uint32(), ctypes.c_uint32()
    rc = _library().nhw_picture_info(b.ctypes.data if b.size else None, b.size, ctypes.byref(w), ctypes.byref(h))
    if rc != NHW_OK:
        raise NhwError(f"not a well-formed .nhwp container (rc={rc})")
    return w.value, h.value


class Encoder:
    """One encoder handle on one GPU.  encode_device() works on torch CUDA tensors already in HBM."""

    def __init__(self, device: int = 0, max_batch: int = 64, device_only: bool = False):
        """device_only: the handle is for encode_device() -- no staging buffers of the host path (nhw_enc_create_ex, NHW_CREATE_DEVICE_ONLY)"""
        import torch
        if not torch.cuda.is_available():
            raise NhwError("no GPU visible: nhwcodec_amd has no CPU path")
        self.torch = torch
        self.lib = load_library()
        self.device = device
        self.max_batch = max_batch
        h = P()
        self._chk(self.lib.nhw_enc_create_ex(device, max_batch, 1 if device_only else 0, ctypes.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise NhwError(f"libnhwhip rc={rc}: {self.lib.nhw_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.free_pinned()        # page-locked buffers handed out by pinned_images() end with the handle
            self.lib.nhw_enc_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_compat(self, glibc_oneshot: bool):
        """False: canonical output (default).  True: reproduce the stock one-image-per-process binary (include/nhw_hip.h)."""
        self._chk(self.lib.nhw_enc_set_compat(self.h, 1 if glibc_oneshot else 0))

    def _stream(self):
        return self.torch.cuda.current_stream(self.device).cuda_stream

    def synth_device(self, n: int, seed_base: int = 0):
        t = self.torch.empty((n, 512, 512, 3), dtype=self.torch.uint8, device=f"cuda:{self.device}")
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_synth_batch_device(self.h, t.data_ptr(), n, seed_base, st))
        return t

    def alloc_out(self, n: int):
        dev = f"cuda:{self.device}"
        return (self.torch.empty((n, OUT_STRIDE), dtype=self.torch.uint8, device=dev),
                self.torch.empty(n, dtype=self.torch.int32, device=dev),
                self.torch.empty(n, dtype=self.torch.int32, device=dev))

    def _device_batch(self, bgr, what):
        """bgr: a contiguous uint8 CUDA tensor [n,512,512,3] on this encoder's device -> n"""
        if not (bgr.is_cuda and bgr.dtype == self.torch.uint8 and bgr.is_contiguous() and bgr.dim() == 4 and tuple(bgr.shape[1:]) == (512, 512, 3)):
            raise NhwError(f"{what} wants a contiguous uint8 CUDA tensor of shape [n, 512, 512, 3]")
        if bgr.device.index != self.device:
            raise NhwError(f"the batch is on cuda:{bgr.device.index}, this encoder on cuda:{self.device}")
        return bgr.shape[0]

    def _device_outputs(self, what, n, out, extra=()):
        """out (None: new tensors), checked: uint8 [n, OUT_STRIDE], int32 sizes [n] and status [n], then an [n] tensor of each dtype in `extra`"""
        t = self.torch
        kinds = [(t.uint8, n * OUT_STRIDE), (t.int32, n), (t.int32, n)] + [(dt, n) for dt in extra]
        if out is None:
            out = self.alloc_out(n) + tuple(t.empty(n, dtype=dt, device=f"cuda:{self.device}") for dt in extra)
        if len(out) != len(kinds):
            raise ValueError(f"{what}: `out` holds {len(out)} tensors, not {len(kinds)}")
        if not all(x.is_cuda and x.device.index == self.device and x.dtype == dt and x.is_contiguous() and x.numel() >= cnt for x, (dt, cnt) in zip(out, kinds)):
            shapes = " / ".join(["uint8 [n, OUT_STRIDE]"] + [f"{str(dt).split('.')[-1]} [n]" for dt, _ in kinds[1:]])
            raise NhwError(f"{what}: output tensors must be contiguous, on this encoder's device, {shapes}")
        return out

    @staticmethod
    def _host_images(images, what):
        """images as a contiguous numpy uint8 [n,512,512,3]"""
        import numpy as np
        images = np.asarray(images)
        if images.dtype != np.uint8 or images.ndim != 4 or images.shape[1:] != (512, 512, 3):
            raise NhwError(f"{what} wants uint8 [n, 512, 512, 3] (BMP file order), got {images.dtype} {images.shape}")
        return np.ascontiguousarray(images)

    def encode_device(self, bgr, quality: int = QUALITY_DEFAULT, out=None):
        """bgr: uint8 CUDA tensor [n,512,512,3] (BMP file order).  Returns (out[n,OUT_STRIDE], sizes[n], status[n]) on device."""
        n = self._device_batch(bgr, "encode_device")
        o, sizes, status = self._device_outputs("encode_device", n, out)
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_batch_device(self.h, bgr.data_ptr(), n, quality, o.data_ptr(), sizes.data_ptr(), status.data_ptr(), st))
        return o, sizes, status

    def encode_tensor_device(self, x, fmt, quality: int = QUALITY_DEFAULT, out=None):
        """encode_device straight from a tensor batch (nhw_enc_batch_device_tensor): x as for tensor_to_bytes_device, on
        this encoder's device.  The files, sizes and status are those of encode_device(tensor_to_bytes_device(x, fmt)), byte for byte; the bytes
        go through a scratch the handle allocates on its first tensor call.  Returns (out[n,OUT_STRIDE], sizes[n], status[n]) on device."""
        what = "encode_tensor_device"
        fmt = _tensor_format(fmt, what)
        n = _tensor_batch(x, fmt, what, self.device)
        if n > self.max_batch:
            raise NhwError(f"{what}: {n} pictures for an encoder of max_batch {self.max_batch}")
        o, sizes, status = self._device_outputs(what, n, out)
        c = fmt.c_struct()
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_batch_device_tensor(self.h, x.data_ptr(), n, ctypes.byref(c), quality, o.data_ptr(), sizes.data_ptr(), status.data_ptr(), st))
        return o, sizes, status

    def encode_grey_device(self, grey, quality: int = QUALITY_DEFAULT, out=None):
        """encode_device from grey pictures (nhw_enc_batch_device_grey): grey, a contiguous, 16-byte aligned uint8 CUDA
        tensor [n, 512, 512], rows in the byte path's order.  File i is byte for byte the file of encode_device on the picture with grey[i] in B,
        G and R; no colour conversion and no 4:2:0 filter runs.  Returns (out[n,OUT_STRIDE], sizes[n], status[n]) on device."""
        what = "encode_grey_device"
        t = self.torch
        if not (isinstance(grey, t.Tensor) and grey.is_cuda and grey.dtype == t.uint8 and grey.is_contiguous() and grey.dim() == 3 and tuple(grey.shape[1:]) == (512, 512)):
            raise NhwError(f"{what} wants a contiguous uint8 CUDA tensor of shape [n, 512, 512]")
        if grey.device.index != self.device:
            raise NhwError(f"the batch is on cuda:{grey.device.index}, this encoder on cuda:{self.device}")
        n = grey.shape[0]
        o, sizes, status = self._device_outputs(what, n, out)
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_batch_device_grey(self.h, grey.data_ptr(), n, quality, o.data_ptr(), sizes.data_ptr(), status.data_ptr(), st))
        return o, sizes, status

    def encode_grey_tensor_device(self, x, fmt, quality: int = QUALITY_DEFAULT, out=None):
        """encode_grey_device straight from a one-channel tensor batch (nhw_enc_batch_device_grey_tensor): x and fmt as for
        tensor_to_grey_bytes_device, on this encoder's device.  The files are those of encode_grey_device(tensor_to_grey_bytes_device(x, fmt))."""
        what = "encode_grey_tensor_device"
        fmt = _tensor_format(fmt, what, grey=True)
        n = _tensor_batch(x, fmt, what, self.device)
        if n > self.max_batch:
            raise NhwError(f"{what}: {n} pictures for an encoder of max_batch {self.max_batch}")
        o, sizes, status = self._device_outputs(what, n, out)
        c = fmt.c_struct()
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_batch_device_grey_tensor(self.h, x.data_ptr(), n, ctypes.byref(c), quality, o.data_ptr(), sizes.data_ptr(), status.data_ptr(), st))
        return o, sizes, status

    def encode_grey(self, pictures, quality: int = QUALITY_DEFAULT):
        """pictures: numpy uint8 [n,512,512] on the host, grey -> list of .nhw byte strings (nhw_enc_batch_grey; raises on a per-image failure)."""
        import numpy as np
        pictures = np.asarray(pictures)
        if pictures.dtype != np.uint8 or pictures.ndim != 3 or pictures.shape[1:] != (512, 512):
            raise NhwError(f"encode_grey wants uint8 [n, 512, 512] (BMP file order), got {pictures.dtype} {pictures.shape}")
        pictures = np.ascontiguousarray(pictures)
        n = pictures.shape[0]
        arena = np.empty(n * OUT_STRIDE, np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_batch_grey(self.h, pictures.ctypes.data, n, quality, arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-image status {status.tolist()}")
        return _split(arena, offs)

    def encode(self, images, quality: int = QUALITY_DEFAULT):
        """images: numpy uint8 [n,512,512,3] on the host -> list of .nhw byte strings (raises on a per-image failure)."""
        import numpy as np
        images = self._host_images(images, "encode")
        n = images.shape[0]
        arena = np.empty(n * OUT_STRIDE, np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_batch(self.h, images.ctypes.data, n, quality, arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-image status {status.tolist()}")
        return _split(arena, offs)

    @staticmethod
    def _ladder(ladder):
        """-> (ctypes int array or None, length); None = the library's default ladder 23, 22, ..., 1"""
        if ladder is None:
            return None, 0
        ladder = [int(q) for q in ladder]
        return (ctypes.c_int * len(ladder))(*ladder), len(ladder)

    def encode_fit_device(self, bgr, max_bytes, ladder=None, out=None):
        """The best picture within a byte budget: for image i the file of the first quality of `ladder` (default 23, 22, ..., 1) whose
        encode succeeds with at most max_bytes[i] bytes, identical to encode_device at that quality (nhw_enc_fit_batch_device).
        bgr as for encode_device; max_bytes: an int for every image, or a contiguous int32 / uint32 CUDA tensor [n] (read as uint32).
        Returns (out[n,OUT_STRIDE], sizes[n], status[n], quality[n]) on the device; status NHW_E_BUDGET where no rung fits (the slot
        then holds the last rung's file).  Waits on the host between rungs: not for graph capture."""
        t = self.torch
        n = self._device_batch(bgr, "encode_fit_device")
        if isinstance(max_bytes, numbers.Integral):
            if max_bytes < 0:
                raise NhwError(f"max_bytes must not be negative, got {max_bytes}")
            budget = t.full((n,), min(int(max_bytes), 2**31 - 1), dtype=t.int32, device=f"cuda:{self.device}")   # (a file is at most OUT_STRIDE bytes)
        else:
            budget = max_bytes
            if not (isinstance(budget, t.Tensor) and budget.dtype in (t.int32, getattr(t, "uint32", t.int32)) and budget.is_cuda
                    and budget.device.index == self.device and budget.is_contiguous() and budget.numel() == n):
                raise NhwError("encode_fit_device: max_bytes must be an int or a contiguous int32 / uint32 tensor [n] on this encoder's device")
        o, sizes, status, quality = self._device_outputs("encode_fit_device", n, out, (t.int32,))
        lad, lad_n = self._ladder(ladder)
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_fit_batch_device(self.h, bgr.data_ptr(), n, budget.data_ptr(), lad, lad_n, o.data_ptr(), sizes.data_ptr(),
                                                        status.data_ptr(), quality.data_ptr(), st))
        return o, sizes, status, quality

    def encode_fit(self, images, max_bytes, ladder=None):
        """images: numpy uint8 [n,512,512,3] on the host; max_bytes: an int or n ints -> (files, qualities, status), lists of n.
        A per-image NHW_E_BUDGET (files[i] = the last rung's file) or NHW_E_CODEBOOK (files[i] = b"") is reported, not raised."""
        import numpy as np
        images = self._host_images(images, "encode_fit")
        n = images.shape[0]
        mb = np.asarray(max_bytes, dtype=np.int64)
        if mb.ndim == 0:
            mb = np.full(n, int(mb), np.int64)
        if mb.shape != (n,) or (mb < 0).any():
            raise NhwError(f"max_bytes must be one non-negative int or {n} of them")
        budget = np.minimum(mb, 2**32 - 1).astype(np.uint32)
        arena = np.empty(n * OUT_STRIDE, np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        lad, lad_n = self._ladder(ladder)
        self._chk(self.lib.nhw_enc_fit_batch(self.h, images.ctypes.data, n, budget.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size,
                                             offs.ctypes.data, status.ctypes.data, quality.ctypes.data))
        return _split(arena, offs), quality.tolist(), status.tolist()

    def _max_sse(self, n, min_psnr, max_sse, what):
        """the per-image SSE targets as a contiguous int64 CUDA tensor [n] (read as uint64) from exactly one of min_psnr / max_sse"""
        import numpy as np
        t = self.torch
        dev = f"cuda:{self.device}"
        if (min_psnr is None) == (max_sse is None):
            raise NhwError(f"{what}: give exactly one of min_psnr and max_sse")
        if min_psnr is not None:
            if isinstance(min_psnr, t.Tensor):
                min_psnr = min_psnr.detach().cpu().numpy()
            m = psnr_to_max_sse(min_psnr)
            if isinstance(m, int):
                return t.full((n,), m, dtype=t.int64, device=dev)
            if m.shape != (n,):
                raise NhwError(f"{what}: min_psnr must be one number or {n} of them")
            return t.from_numpy(np.ascontiguousarray(m)).to(dev)
        if isinstance(max_sse, numbers.Integral):
            if max_sse < 0:
                raise NhwError(f"max_sse must not be negative, got {max_sse}")
            return t.full((n,), min(int(max_sse), 2**63 - 1), dtype=t.int64, device=dev)
        if not (isinstance(max_sse, t.Tensor) and max_sse.dtype in (t.int64, getattr(t, "uint64", t.int64)) and max_sse.is_cuda
                and max_sse.device.index == self.device and max_sse.is_contiguous() and max_sse.numel() == n):
            raise NhwError(f"{what}: max_sse must be an int or a contiguous int64 / uint64 tensor [n] on this encoder's device")
        return max_sse

    def _decoder(self, decoder, n, what):
        if not isinstance(decoder, Decoder) or not getattr(decoder, "h", None):
            raise NhwError(f"{what} needs an open Decoder")
        if decoder.device != self.device:
            raise NhwError(f"{what}: the decoder is on cuda:{decoder.device}, this encoder on cuda:{self.device}")
        if decoder.max_batch < n:
            raise NhwError(f"{what}: the decoder's max_batch {decoder.max_batch} is below n = {n}")
        return decoder.h

    def encode_fit_psnr_device(self, bgr, decoder, min_psnr=None, max_sse=None, ladder=None, out=None):
        """The smallest quality that looks good enough: for image i the file of the first quality of `ladder` (default 1, 2, ..., 23) whose
        encode succeeds and whose decode by `decoder` (the bit-exact device decoder) is within image i's target, identical to encode_device at
        that quality (nhw_enc_fit_sse_batch_device).  The target is given by exactly one of min_psnr (dB: a float, or float64 values per
        image; see psnr_to_max_sse) and max_sse (the largest sum of squared differences over the picture's 786432 bytes: an int, or a
        contiguous int64 / uint64 CUDA tensor [n], read as uint64).  bgr as for encode_device.
        Returns (out[n,OUT_STRIDE], sizes[n], status[n], quality[n], sse[n]) on the device: sse int64, the achieved SSE (UINT64_MAX, i.e.
        -1, where there is no decoded picture).  status NHW_E_BUDGET where no rung meets the target (the slot then holds the last rung's
        file).  Waits on the host between rungs: not for graph capture."""
        t = self.torch
        what = "encode_fit_psnr_device"
        n = self._device_batch(bgr, what)
        dh = self._decoder(decoder, n, what)
        target = self._max_sse(n, min_psnr, max_sse, what)
        o, sizes, status, quality, sse = self._device_outputs(what, n, out, (t.int32, t.int64))
        lad, lad_n = self._ladder(ladder)
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_enc_fit_sse_batch_device(self.h, dh, bgr.data_ptr(), n, target.data_ptr(), lad, lad_n, o.data_ptr(), sizes.data_ptr(),
                                                            status.data_ptr(), quality.data_ptr(), sse.data_ptr(), st))
        return o, sizes, status, quality, sse

    def encode_fit_psnr(self, images, decoder, min_psnr, ladder=None):
        """images: numpy uint8 [n,512,512,3] on the host; min_psnr: dB, one number or n of them -> (files, qualities, status, sse), lists of n.
        A per-image NHW_E_BUDGET (files[i] = the last rung's file) or NHW_E_CODEBOOK (files[i] = b"", sse 2**64 - 1) is reported, not raised."""
        import numpy as np
        images = self._host_images(images, "encode_fit_psnr")
        n = images.shape[0]
        dh = self._decoder(decoder, n, "encode_fit_psnr")
        target = psnr_to_max_sse(min_psnr)
        target = np.full(n, target, np.uint64) if isinstance(target, int) else target.astype(np.uint64)
        if target.shape != (n,):
            raise NhwError(f"encode_fit_psnr: min_psnr must be one number or {n} of them")
        arena = np.empty(n * OUT_STRIDE, np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        sse = np.empty(n, np.uint64)
        lad, lad_n = self._ladder(ladder)
        self._chk(self.lib.nhw_enc_fit_sse_batch(self.h, dh, images.ctypes.data, n, target.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size,
                                                 offs.ctypes.data, status.ctypes.data, quality.ctypes.data, sse.ctypes.data))
        return _split(arena, offs), quality.tolist(), status.tolist(), [int(x) for x in sse]

    def fit_stats(self) -> FitStats:
        s = FitStats()
        self._chk(self.lib.nhw_enc_last_fit_stats(self.h, ctypes.byref(s)))
        return s

    def encode_tiled(self, big, quality: int = QUALITY_DEFAULT):
        """a picture whose sides are multiples of 512 -> (list of .nhw byte strings, one per tile, row-major, (ny, nx)); `nhw-enc --tiles`"""
        tiles, shape = tile_images(big)
        return self.encode(tiles, quality), shape

    @staticmethod
    def _host_pictures(pictures, what, grey=False):
        """a list of numpy uint8 [H, W, 3] ([H, W] with grey) -> (n, packed blob, in_off, width, height, tiles, an output arena that holds every container)"""
        import numpy as np
        form = "[H, W]" if grey else "[H, W, 3]"
        if not isinstance(pictures, (list, tuple)) or not pictures:
            raise NhwError(f"{what} wants a non-empty list of uint8 {form} arrays")
        arrs = [np.ascontiguousarray(p) for p in pictures]
        for i, a in enumerate(arrs):
            if a.dtype != np.uint8 or (a.ndim != 2 if grey else a.ndim != 3 or a.shape[2] != 3):
                raise NhwError(f"{what}: picture {i} is not uint8 {form}, got {a.dtype} {a.shape}")
            picture_tiles(a.shape[1], a.shape[0])
        n = len(arrs)
        width = np.array([a.shape[1] for a in arrs], np.uint32)
        height = np.array([a.shape[0] for a in arrs], np.uint32)
        in_off = np.zeros(n + 1, np.uint64)
        in_off[1:] = np.cumsum([a.size for a in arrs])
        blob = np.concatenate([a.reshape(-1) for a in arrs])
        tiles = sum(picture_tiles(int(w), int(h)) for w, h in zip(width, height))
        arena = np.empty(16 * n + tiles * (4 + OUT_STRIDE), np.uint8)
        return n, blob, in_off, width, height, tiles, arena

    def encode_pictures(self, pictures, quality: int = QUALITY_DEFAULT):
        """pictures: a list of numpy uint8 [H, W, 3] (BMP file row order, sides 1..65535) -> a list of .nhwp containers (bytes): every
        picture padded to whole tiles on the device, the tiles encoded in chunks of max_batch (nhw_enc_pictures).  Raises on a per-picture
        failure, like encode."""
        import numpy as np
        n, blob, in_off, width, height, _, arena = self._host_pictures(pictures, "encode_pictures")
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_pictures(self.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n, quality,
                                            arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-picture status {status.tolist()}")
        return _split(arena, offs)

    def encode_pictures_grey(self, pictures, quality: int = QUALITY_DEFAULT):
        """encode_pictures from grey pictures (nhw_enc_pictures_grey): a list of numpy uint8 [H, W] -> a list of .nhwp
        containers, each byte for byte the container of the picture with its bytes in B, G and R; Decoder.decode_pictures_grey reads them."""
        import numpy as np
        n, blob, in_off, width, height, _, arena = self._host_pictures(pictures, "encode_pictures_grey", grey=True)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_pictures_grey(self.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n, quality,
                                                 arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-picture status {status.tolist()}")
        return _split(arena, offs)

    def encode_pictures_resized(self, pictures, size, quality: int = QUALITY_DEFAULT):
        """encode_pictures with the area filter in front (nhw_enc_pictures_resized): pictures as there, size = (out_h,
        out_w) of 1 .. 4096 each -> a list of .nhwp containers of out_w x out_h pictures: thumbnails, a fixed-resolution set.  Picture i is
        resized on the device under the area rule (no mirror) and container i is encode_pictures' for that picture, byte for byte.  A picture
        more than AREA_MAX_REDUCTION times the output along a side is refused.  Raises on a per-picture failure."""
        import numpy as np
        what = "encode_pictures_resized"
        out_h, out_w = _crop_size(size, what)
        n, blob, in_off, width, height, _, _ = self._host_pictures(pictures, what)
        for i in range(n):
            _filter_limit("area", int(width[i]), int(height[i]), out_w, out_h, what, f"picture {i}")
        arena = np.empty(n * (16 + picture_tiles(out_w, out_h) * (4 + OUT_STRIDE)), np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_pictures_resized(self.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n, out_w, out_h, quality,
                                                    arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-picture status {status.tolist()}")
        return _split(arena, offs)

    def encode_resized_device(self, pictures, quality: int = QUALITY_DEFAULT, out=None, filter="area"):
        """Any photo to one .nhw file: pictures, a list of at most max_batch uint8 CUDA tensors [H, W, 3] as for tile_pictures_device (crop views
        work), each resized to one 512 x 512 picture under the area rule (resize_to_tensor_device with filter="area")
        and encoded by encode_device -> (out[n,OUT_STRIDE], sizes[n], status[n]) on device, the files of encode_device on the rule's
        pictures, byte for byte.  filter: "area", or "cubic" for the cubic rule, passed on to the resize."""
        what = "encode_resized_device"
        _filter(filter, what)
        if not isinstance(pictures, (list, tuple)) or not 1 <= len(pictures) <= self.max_batch:
            raise NhwError(f"{what} wants a list of 1 .. max_batch = {self.max_batch} uint8 CUDA tensors [H, W, 3]")
        dev = getattr(pictures[0], "device", None)                   # (the resize checks that all pictures are on one device)
        if dev is not None and dev.type == "cuda" and dev.index != self.device:
            raise NhwError(f"the pictures are on cuda:{dev.index}, this encoder on cuda:{self.device}")
        bgr = resize_to_tensor_device(pictures, (512, 512), TensorFormat("uint8", "HWC", "BGR", "file"), filter=filter)
        return self.encode_device(bgr, quality, out)

    def encode_pictures_fit(self, pictures, max_bytes, ladder=None):
        """The best .nhwp within a byte budget (nhw_enc_fit_pictures): pictures as for encode_pictures; max_bytes: an int or one per picture,
        the budget for the whole container -> (containers, qualities, status), lists of n.  Picture i gets the container of the first quality
        of `ladder` (default 23, 22, ..., 1) at which all its tiles encode and the container fits, identical to encode_pictures at that quality;
        every tile of a picture has that one quality.  A per-picture NHW_E_BUDGET (the last rung's container) or NHW_E_CODEBOOK (b"") is
        reported, not raised."""
        import numpy as np
        n, blob, in_off, width, height, _, arena = self._host_pictures(pictures, "encode_pictures_fit")
        mb = np.asarray(max_bytes, dtype=object)
        mb = np.full(n, mb.item(), dtype=object) if mb.ndim == 0 else mb
        if mb.shape != (n,) or not all(isinstance(x, numbers.Integral) and x >= 0 for x in mb):
            raise NhwError(f"max_bytes must be one non-negative int or {n} of them")
        budget = np.array([min(int(x), 2**64 - 1) for x in mb], np.uint64)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        lad, lad_n = self._ladder(ladder)
        self._chk(self.lib.nhw_enc_fit_pictures(self.h, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n,
                                                budget.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data,
                                                quality.ctypes.data))
        return _split(arena, offs), quality.tolist(), status.tolist()

    def encode_pictures_fit_psnr(self, pictures, decoder, min_psnr, ladder=None):
        """The smallest quality whose .nhwp looks good enough (nhw_enc_fit_sse_pictures): pictures as for encode_pictures; min_psnr: dB, one
        number or one per picture, over the picture's own pixels (picture_psnr_to_max_sse) -> (containers, qualities, status, sse), lists of
        n.  Picture i gets the container of the first quality of `ladder` (default 1, 2, ..., 23) whose decode by `decoder` reaches the target,
        identical to encode_pictures at that quality; sse[i] is the SSE a user measures between decode_pictures of it and the picture.  A
        per-picture NHW_E_BUDGET (the last rung's container) or NHW_E_CODEBOOK (b"", sse 2**64 - 1) is reported, not raised."""
        import numpy as np
        n, blob, in_off, width, height, tiles, arena = self._host_pictures(pictures, "encode_pictures_fit_psnr")
        dh = self._decoder(decoder, min(self.max_batch, tiles), "encode_pictures_fit_psnr")
        db = np.asarray(min_psnr, dtype=object)
        db = [db.item()] * n if db.ndim == 0 else list(db)
        if len(db) != n:
            raise NhwError(f"encode_pictures_fit_psnr: min_psnr must be one number or {n} of them")
        target = np.array([picture_psnr_to_max_sse(float(x) if isinstance(x, numbers.Real) else x, int(w), int(h))
                           for x, w, h in zip(db, width, height)], np.uint64)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        sse = np.empty(n, np.uint64)
        lad, lad_n = self._ladder(ladder)
        self._chk(self.lib.nhw_enc_fit_sse_pictures(self.h, dh, blob.ctypes.data, in_off.ctypes.data, width.ctypes.data, height.ctypes.data, n,
                                                    target.ctypes.data, lad, lad_n, arena.ctypes.data, arena.size, offs.ctypes.data,
                                                    status.ctypes.data, quality.ctypes.data, sse.ctypes.data))
        return _split(arena, offs), quality.tolist(), status.tolist(), [int(x) for x in sse]

    def timing(self) -> Timing:
        t = Timing()
        self._chk(self.lib.nhw_enc_last_timing(self.h, ctypes.byref(t)))
        return t

    def encode_synthetic(self, n: int, seed_base: int, quality: int = QUALITY_DEFAULT):
        """SURVEY 8(d) images seed_base.. generated on the device, encoded, files brought to the host (`nhw-enc --synthetic`)."""
        import numpy as np
        arena = np.empty(n * OUT_STRIDE, np.uint8)
        offs = np.empty(n + 1, np.uint64)
        status = np.empty(n, np.int32)
        self._chk(self.lib.nhw_enc_synth_batch(self.h, n, seed_base, quality, arena.ctypes.data, arena.size, offs.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-image status {status.tolist()}")
        return _split(arena, offs)

    def pinned_images(self, n: int):
        """uint8 [n,512,512,3] in page-locked host memory (nhw_host_alloc): encode() uploads such a batch by DMA at PCIe speed while the
        chunk before is being encoded.  Keep the returned array alive only as long as this encoder; free with free_pinned()."""
        import numpy as np
        p = self.lib.nhw_host_alloc(n * IMG_BYTES)
        if not p:
            raise NhwError("nhw_host_alloc failed")
        buf = (ctypes.c_uint8 * (n * IMG_BYTES)).from_address(p)
        a = np.frombuffer(buf, np.uint8).reshape(n, 512, 512, 3)
        self._pinned = getattr(self, "_pinned", []) + [p]
        return a

    def free_pinned(self):
        for p in getattr(self, "_pinned", []):
            self.lib.nhw_host_free(p)
        self._pinned = []


def _split(arena, offs):
    """the files of a host-path arena: file i is arena[offs[i]:offs[i + 1]] -> a list of bytes"""
    return [arena[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(offs) - 1)]


def tile_images(big):
    """a uint8 [512*ny, 512*nx, 3] picture (BMP file row order) -> ([ny*nx, 512, 512, 3] independent tiles, row-major, (ny, nx)).
    Every tile is a picture of its own to the codec: no state crosses a tile edge, in either direction."""
    import numpy as np
    big = np.asarray(big)
    if big.dtype != np.uint8 or big.ndim != 3 or big.shape[2] != 3 or big.shape[0] < 512 or big.shape[1] < 512 or big.shape[0] % 512 or big.shape[1] % 512:
        raise NhwError(f"tiling wants uint8 [512*ny, 512*nx, 3], got {big.dtype} {big.shape}")
    ny, nx = big.shape[0] // 512, big.shape[1] // 512
    return np.ascontiguousarray(big.reshape(ny, 512, nx, 512, 3).transpose(0, 2, 1, 3, 4)).reshape(ny * nx, 512, 512, 3), (ny, nx)


def untile_images(tiles, ny: int, nx: int):
    """the inverse of tile_images"""
    import numpy as np
    tiles = np.asarray(tiles)
    if tiles.shape != (ny * nx, 512, 512, 3):
        raise NhwError(f"untile wants [{ny * nx}, 512, 512, 3], got {tiles.shape}")
    return np.ascontiguousarray(tiles.reshape(ny, nx, 512, 512, 3).transpose(0, 2, 1, 3, 4)).reshape(ny * 512, nx * 512, 3)


class _OnTorchStream:
    """Stream-ordered launch next to torch: the C ABI takes a hipStream_t and reads NULL as "the handle's own stream", which torch's
    default stream (handle 0) would select by accident.  On the default stream the work goes to a side stream that waits for it
    and that it waits for afterwards, so callers see ordinary stream semantics either way."""

    def __init__(self, owner):
        self.o = owner

    def __enter__(self):
        t, o = self.o.torch, self.o
        self.cur = t.cuda.current_stream(o.device)
        if self.cur.cuda_stream != 0:
            self.side = None
            return self.cur.cuda_stream
        if getattr(o, "_side", None) is None:
            o._side = t.cuda.Stream(o.device)
        self.side = o._side
        self.side.wait_stream(self.cur)
        return self.side.cuda_stream

    def __exit__(self, *exc):
        if self.side is not None:
            self.cur.wait_stream(self.side)
        return False


class DecTiming(ctypes.Structure):
    _fields_ = [(n, ctypes.c_float) for n in ("total_ms", "entropy_ms", "recon_ms")]


class Decoder:
    """One decoder handle on one GPU: mirror of the reference's decode_image + write_image_bmp
    (decoder/nhw_decoder.c:54, decoder/nhw_decoder_cli.c:108) for batches of .nhw files."""

    def __init__(self, device: int = 0, max_batch: int = 64):
        import torch
        if not torch.cuda.is_available():
            raise NhwError("no GPU visible: nhwcodec_amd has no CPU path")
        self.torch = torch
        self.lib = L = load_library()
        L.nhw_dec_last_error.restype = ctypes.c_char_p
        L.nhw_dec_create.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.POINTER(P)]
        L.nhw_dec_destroy.argtypes = [P]
        L.nhw_dec_batch_device.argtypes = [P, P, P, P, ctypes.c_int, P, P, P, P]
        L.nhw_dec_batch.argtypes = [P, P, P, ctypes.c_int, P, P, P]
        L.nhw_dec_bmp_header.argtypes = [P]
        L.nhw_dec_last_timing.argtypes = [P, ctypes.POINTER(DecTiming)]
        L.nhw_dec_debug_stop_after.argtypes = [P, ctypes.c_int]
        L.nhw_dec_debug_read.argtypes = [P, ctypes.c_int, ctypes.c_int, P, ctypes.c_size_t]
        self.device = device
        self.max_batch = max_batch
        h = P()
        self._chk(L.nhw_dec_create(device, max_batch, ctypes.byref(h)))
        self.h = h

    def _chk(self, rc):
        if rc != 0:
            raise NhwError(f"libnhwhip rc={rc}: {self.lib.nhw_dec_last_error().decode()}")

    def close(self):
        if getattr(self, "h", None):
            self.lib.nhw_dec_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bmp_header(self) -> bytes:
        h = ctypes.create_string_buffer(54)
        self.lib.nhw_dec_bmp_header(ctypes.cast(h, P))
        return h.raw

    def decode_tiled(self, files, ny: int, nx: int):
        """the tiles written by encode_tiled -> uint8 [512*ny, 512*nx, 3]; `nhw-dec --tiles`"""
        if len(files) != ny * nx:
            raise NhwError(f"{len(files)} files for {ny} x {nx} tiles")
        px, _ = self.decode(files)
        return untile_images(px, ny, nx)

    def timing(self) -> DecTiming:
        t = DecTiming()
        self._chk(self.lib.nhw_dec_last_timing(self.h, ctypes.byref(t)))
        return t

    def _device_files(self, arena, offsets, lengths, what, limit=True):
        """the checked files of a decode_*_device call: arena uint8, offsets int64 [n], lengths int32 [n], contiguous, on this decoder's device
        -> n (limit: at most max_batch)"""
        t = self.torch
        for name, x, dt in (("arena", arena, t.uint8), ("offsets", offsets, t.int64), ("lengths", lengths, t.int32)):
            if not (isinstance(x, t.Tensor) and x.is_cuda and x.device.index == self.device and x.dtype == dt and x.is_contiguous()):
                raise NhwError(f"{what}: `{name}` must be a contiguous {dt} tensor on cuda:{self.device}")
        n = offsets.numel()
        if lengths.numel() != n or n < 1:
            raise NhwError(f"{what}: offsets and lengths must have one entry per file")
        if limit and n > self.max_batch:
            raise NhwError(f"{what}: {n} files for a decoder of max_batch {self.max_batch}")
        return n

    def _device_out(self, out, what, dtype, shape, align, wants):
        """the checked `out` of a decode_*_device call (None: a new tensor of `shape`): contiguous, of dtype, on this decoder's device, at least
        prod(shape) elements at an address that is a multiple of align; wants: the error's words for that -> (out, its first prod(shape)
        elements as `shape`, new status [n] and quality [n])"""
        t = self.torch
        dev = f"cuda:{self.device}"
        count = 1
        for v in shape:
            count *= v
        if out is None:
            out = t.empty(shape, dtype=dtype, device=dev)
        elif not (isinstance(out, t.Tensor) and out.is_cuda and out.device.index == self.device and out.dtype == dtype and out.is_contiguous()
                  and out.numel() >= count and out.data_ptr() % align == 0):
            raise NhwError(f"{what}: `out` must be a {wants} on this decoder's device")
        px = out if tuple(out.shape) == tuple(shape) else out.reshape(-1)[:count].view(shape)
        return out, px, t.empty(shape[0], dtype=t.int32, device=dev), t.empty(shape[0], dtype=t.int32, device=dev)

    def decode_device(self, arena, offsets, lengths, out=None):
        """arena: uint8 CUDA tensor holding the files; offsets: int64 CUDA tensor [n]; lengths: int32 CUDA tensor [n]
        (the encoder's output arena with offsets i*OUT_STRIDE and its sizes tensor fits as is).
        Returns (pixels[n,512,512,3], status[n], quality[n]) on the device."""
        n = self._device_files(arena, offsets, lengths, "decode_device", limit=False)
        out, _, status, quality = self._device_out(out, "decode_device", self.torch.uint8, (n, 512, 512, 3), 1, "contiguous uint8 tensor of n*786432 bytes")
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_dec_batch_device(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, out.data_ptr(), status.data_ptr(),
                                                    quality.data_ptr(), st))
        return out, status, quality

    def decode_scaled_device(self, arena, offsets, lengths, scale, out=None):
        """decode_device at scale 1, 2 or 4 (nhw_dec_batch_device_scaled): the half-scale (256 x 256, exact 4:4:4) or
        quarter-scale (128 x 128) picture every file holds, without the level-1 synthesis.  Arguments as for decode_device; out: a contiguous
        uint8 tensor of at least n * 3 * S * S bytes, S = 512 // scale.  Returns (pixels[n, S, S, 3], status[n], quality[n]) on the device;
        status and quality are those of the full decode.  Scale 1 is decode_device."""
        what = "decode_scaled_device"
        scale = _scale(scale, what)
        side = 512 // scale
        n = self._device_files(arena, offsets, lengths, what)
        out, px, status, quality = self._device_out(out, what, self.torch.uint8, (n, side, side, 3), 8,
                                                    f"contiguous, 8-byte aligned uint8 tensor of n*{3 * side * side} bytes")
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_dec_batch_device_scaled(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, scale, out.data_ptr(),
                                                           status.data_ptr(), quality.data_ptr(), st))
        return px, status, quality

    def _ops_tables(self, n, flips, colours, tones, what, channels):
        """_decode_ops' tables on this decoder's device -> the three tensors (None where the argument is); the caller keeps them until its call is
        queued on torch's current stream, where their memory's reuse is ordered behind it"""
        t = self.torch
        dev = t.device("cuda", self.device)
        flags, maps, tabs = _decode_ops(n, flips, colours, tones, what, channels)
        return (t.from_numpy(flags).to(dev) if flags is not None else None, _device_table(maps, dev) if maps is not None else None,
                _device_tones(tabs, dev, what) if tabs is not None else None)

    def decode_tensor_device(self, arena, offsets, lengths, fmt, scale=1, out=None, flips=None, colours=None, tones=None):
        """decode_scaled_device straight into a tensor format (nhw_dec_batch_device_tensor): the last kernel stores
        fmt's element type, layout, channel order and row direction from the registers that hold the pixel, with no pass over the bytes.
        Arguments as for decode_scaled_device; fmt: a TensorFormat; out: a contiguous, 16-byte aligned tensor of fmt.dtype with at least
        n * 3 * S * S elements, S = 512 // scale.  Returns (tensor [n, 3, S, S] or [n, S, S, 3], status[n], quality[n]) on the device; a
        refused file's slot is left untouched.
        flips, colours, tones: the per-sample operations in the same store (nhw_dec_batch_device_tensor_ops), each None or
        as the crop calls take it -- flips: one boolean or flag byte a file ("mirror left-right"); colours: ONE colour map for all files or one a
        file, a 3 x 4 matrix of floats on (R, G, B, 1) as colour_matrix makes it or the twelve integers of colour_fixed; tones: one tone table a
        file, uint8 [3, 256] on R, G, B as the tone_* builders make it, or the uint8 CUDA tensor [n, 768] of tone_from_hist_device.  The order
        is fixed: the plain decode's pixel, mirror, colour map, tone table, then fmt's value rule, channel order, layout and rows.  All are
        checked on the host before anything is launched; with all three None the call is the plain one."""
        what = "decode_tensor_device"
        fmt = _tensor_format(fmt, what)
        scale = _scale(scale, what)
        side = 512 // scale
        ops = flips is not None or colours is not None or tones is not None
        if ops and hasattr(lengths, "shape") and len(lengths.shape) == 1:   # the tables' lengths and limits before a device is looked at
            _decode_ops(int(lengths.shape[0]), flips, colours, tones, what)
        n = self._device_files(arena, offsets, lengths, what)
        out, px, status, quality = self._device_out(out, what, fmt.dtype, (n,) + fmt.shape(side, side), 16,
                                                    f"contiguous, 16-byte aligned {fmt.dtype} tensor of n*{3 * side * side} elements")
        c = fmt.c_struct()
        if ops:
            tabs = self._ops_tables(n, flips, colours, tones, what, 3)
            with _OnTorchStream(self) as st:
                self._chk(self.lib.nhw_dec_batch_device_tensor_ops(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, scale, ctypes.byref(c),
                                                                   *(x.data_ptr() if x is not None else None for x in tabs),
                                                                   out.data_ptr(), status.data_ptr(), quality.data_ptr(), st))
            return px, status, quality
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_dec_batch_device_tensor(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, scale, ctypes.byref(c),
                                                           out.data_ptr(), status.data_ptr(), quality.data_ptr(), st))
        return px, status, quality

    def decode_grey_device(self, arena, offsets, lengths, scale=1, fmt=None, out=None, flips=None, colours=None, tones=None):
        """decode_scaled_device as grey (nhw_dec_batch_device_grey): the luma alone, through the grey table of the
        file's quality (grey_table), one channel; the chroma planes are not decoded.  Arguments as for decode_scaled_device.  Without fmt:
        (uint8 pixels [n, S, S], rows in file order, status[n], quality[n]), S = 512 // scale.  With fmt, a TensorFormat of channels "GREY":
        (tensor [n, 1, S, S] or [n, S, S, 1] of fmt.dtype, status, quality).  out: a contiguous, 16-byte aligned tensor of that dtype with at
        least n * S * S elements.  Status and quality are those of the colour decode; a refused file's slot is left untouched.
        flips, colours, tones: as for decode_tensor_device, in their one-channel forms (nhw_dec_batch_device_grey_ops) --
        colours: ONE pair (gain, offset) for all files or one a file; tones: one table uint8 [256] a file (or the CUDA tensor [n, 768], of which
        a file's first 256 bytes are read).  The order is fixed: the grey byte of the plain decode, mirror, map, table, then the value rule and
        rows.  With all three None the call is the plain one."""
        what = "decode_grey_device"
        if fmt is not None:
            _tensor_format(fmt, what, grey=True)
        scale = _scale(scale, what)
        side = 512 // scale
        ops = flips is not None or colours is not None or tones is not None
        if ops and hasattr(lengths, "shape") and len(lengths.shape) == 1:
            _decode_ops(int(lengths.shape[0]), flips, colours, tones, what, 1)
        n = self._device_files(arena, offsets, lengths, what)
        dtype = self.torch.uint8 if fmt is None else fmt.dtype
        out, px, status, quality = self._device_out(out, what, dtype, (n, side, side) if fmt is None else (n,) + fmt.shape(side, side), 16,
                                                    f"contiguous, 16-byte aligned {dtype} tensor of n*{side * side} elements")
        c = None if fmt is None else fmt.c_struct()
        if ops:
            tabs = self._ops_tables(n, flips, colours, tones, what, 1)
            with _OnTorchStream(self) as st:
                self._chk(self.lib.nhw_dec_batch_device_grey_ops(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, scale,
                                                                 None if c is None else ctypes.byref(c), *(x.data_ptr() if x is not None else None for x in tabs),
                                                                 out.data_ptr(), status.data_ptr(), quality.data_ptr(), st))
            return px, status, quality
        with _OnTorchStream(self) as st:
            self._chk(self.lib.nhw_dec_batch_device_grey(self.h, arena.data_ptr(), offsets.data_ptr(), lengths.data_ptr(), n, scale,
                                                         None if c is None else ctypes.byref(c), out.data_ptr(), status.data_ptr(), quality.data_ptr(), st))
        return px, status, quality

    def _scaled_host(self, files, scale, what, call, channels):
        """decode_scaled and decode_grey: call = the C entry -> (uint8 [n, S, S] + channels, quality list)"""
        import numpy as np
        scale = _scale(scale, what)
        side = 512 // scale
        if not isinstance(files, (list, tuple)) or not files or not all(isinstance(f, (bytes, bytearray, memoryview)) for f in files):
            raise NhwError(f"{what} wants a non-empty list of .nhw byte strings")
        n = len(files)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in files])
        blob = np.frombuffer(b"".join(bytes(f) for f in files) + b"\0", np.uint8)
        out = np.empty((n, side, side) + channels, np.uint8)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        self._chk(call(self.h, blob.ctypes.data, offs.ctypes.data, n, scale, out.ctypes.data, status.ctypes.data, quality.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-file status {status.tolist()}")
        return out, quality.tolist()

    def decode_scaled(self, files, scale):
        """decode at scale 1, 2 or 4 (nhw_dec_batch_scaled): files, a list of .nhw byte strings of any length (decoded in chunks of max_batch) ->
        (uint8 [n, S, S, 3] with S = 512 // scale, quality list).  Raises on a file the decoder refuses."""
        return self._scaled_host(files, scale, "decode_scaled", self.lib.nhw_dec_batch_scaled, (3,))

    def decode_grey(self, files, scale=1):
        """decode_scaled as grey (nhw_dec_batch_grey) -> (uint8 [n, S, S], rows in file order, quality list)."""
        return self._scaled_host(files, scale, "decode_grey", self.lib.nhw_dec_batch_grey, ())

    def _pictures_host(self, containers, scale, call):
        """decode_pictures and decode_pictures_scaled: call(blob, offsets, n, out, out_off, status) -> rc"""
        import numpy as np
        n = len(containers)
        shapes = [scaled_size(*picture_info(c), scale) for c in containers]
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([len(c) for c in containers])
        blob = np.frombuffer(b"".join(bytes(c) for c in containers), np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        out_off[1:] = np.cumsum([3 * w * h for w, h in shapes])
        out = np.empty(int(out_off[n]), np.uint8)
        status = np.empty(n, np.int32)
        self._chk(call(blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data, out_off.ctypes.data, status.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-container status {status.tolist()}")
        return [out[int(out_off[i]):int(out_off[i + 1])].reshape(h, w, 3) for i, (w, h) in enumerate(shapes)]

    def decode_pictures_scaled(self, containers, scale):
        """decode_pictures at scale 1, 2 or 4 (nhw_dec_pictures_scaled): a list of .nhwp containers (bytes) -> a list of numpy uint8
        [ceil(H / scale), ceil(W / scale), 3], each assembled on the device from the scaled decode of its tiles: the overview of a large picture
        without the level-1 synthesis of a single tile.  Raises on a malformed container or a tile the decoder refuses."""
        scale = _scale(scale, "decode_pictures_scaled")
        if not isinstance(containers, (list, tuple)) or len(containers) < 1:
            raise NhwError("decode_pictures_scaled wants a non-empty list of containers")
        return self._pictures_host(containers, scale, lambda *a: self.lib.nhw_dec_pictures_scaled(self.h, *a[:3], scale, *a[3:]))

    def decode_pictures(self, containers):
        """containers: a list of .nhwp containers (bytes) -> a list of numpy uint8 [H, W, 3]: the tiles decoded in chunks of max_batch and
        cropped on the device (nhw_dec_pictures).  Raises on a malformed container or a tile the decoder refuses."""
        if len(containers) < 1:
            raise NhwError("decode_pictures wants a non-empty list of containers")
        return self._pictures_host(containers, 1, lambda *a: self.lib.nhw_dec_pictures(self.h, *a))

    def _region_args(self, containers, rects, what):
        """the packed containers and the checked nhw_rect table of a region call -> (blob, offsets, rect table)"""
        import numpy as np
        if len(containers) < 1 or len(rects) < 1:
            raise NhwError(f"{what} wants a non-empty list of containers and a non-empty list of (container, x, y, w, h)")
        offs = np.zeros(len(containers) + 1, np.uint64)
        offs[1:] = np.cumsum([len(c) for c in containers])
        blob = np.frombuffer(b"".join(bytes(c) for c in containers), np.uint8)
        table = np.zeros(len(rects), RECT_DTYPE)
        for i, r in enumerate(rects):
            if len(r) != 5 or not all(isinstance(v, numbers.Integral) and 0 <= v <= 0xFFFFFFFF for v in r):
                raise NhwError(f"{what}: rect {i} must be (container, x, y, w, h), integers of 32 bits, got {r!r}")
            table[i] = tuple(int(v) for v in r)
        return blob, offs, table

    def _region_raise(self, status):
        if (status != 0).any():
            raise NhwError(f"per-region status {status.tolist()}")

    def _regions_host(self, containers, rects, what, call, channels=3):
        """the host form of a region or window call: call(blob, offsets, n containers, rect table, n, out, out_off, status) -> rc;
        channels=1: a grey call's [h, w] arrays"""
        import numpy as np
        blob, offs, table = self._region_args(containers, rects, what)
        n = len(table)
        out_off = np.zeros(n + 1, np.uint64)
        out_off[1:] = np.cumsum(channels * table["width"].astype(np.uint64) * table["height"].astype(np.uint64))
        out = np.empty(max(int(out_off[n]), 1), np.uint8)
        status = np.empty(n, np.int32)
        self._chk(call(blob.ctypes.data, offs.ctypes.data, len(containers), table.ctypes.data, n, out.ctypes.data, out_off.ctypes.data, status.ctypes.data))
        self._region_raise(status)
        return [out[int(out_off[i]):int(out_off[i + 1])].reshape((int(r["height"]), int(r["width"])) + ((3,) if channels == 3 else ())) for i, r in enumerate(table)]

    def _regions_device(self, containers, rects, out, what, call, channels=3):
        """the device form: call(blob, offsets, n containers, rect table, n, addresses, pitches, status) -> rc; channels=1: a grey call's
        [h, w] tensors with strides (pitch >= w, 1)"""
        import numpy as np
        t = self.torch
        blob, offs, table = self._region_args(containers, rects, what)
        n = len(table)
        dev = t.device("cuda", self.device)
        C = channels
        last = (3,) if C == 3 else ()
        if out is None:
            out = [t.empty((int(r["height"]), int(r["width"])) + last, dtype=t.uint8, device=dev) for r in table]
        elif not isinstance(out, (list, tuple)) or len(out) != n:
            raise NhwError(f"{what}: `out` must be a list of {n} tensors")
        addr, pitch = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        for i, (x, r) in enumerate(zip(out, table)):
            h, w = int(r["height"]), int(r["width"])
            if not (isinstance(x, t.Tensor) and x.is_cuda and x.device == dev and x.dtype == t.uint8 and tuple(x.shape) == (h, w) + last):
                raise NhwError(f"{what}: out[{i}] is not a uint8 tensor {list((h, w) + last)} on {dev}")
            if C == 1 and ((w > 1 and x.stride(1) != 1) or (h > 1 and x.stride(0) < w)):
                raise NhwError(f"{what}: out[{i}] must have strides (pitch >= w, 1), got {tuple(x.stride())}")
            if C == 3 and (x.stride(2) != 1 or (w > 1 and x.stride(1) != 3) or (h > 1 and x.stride(0) < 3 * w)):
                raise NhwError(f"{what}: out[{i}] must have strides (pitch >= 3 w, 3, 1), got {tuple(x.stride())}")
            addr[i], pitch[i] = x.data_ptr(), x.stride(0) if h > 1 else C * w
        status = np.empty(n, np.int32)
        t.cuda.current_stream(dev).synchronize()                     # the call runs on the handle's own stream and waits for it
        self._chk(call(blob.ctypes.data, offs.ctypes.data, len(containers), table.ctypes.data, n, addr.ctypes.data, pitch.ctypes.data, status.ctypes.data))
        self._region_raise(status)
        return list(out)

    def decode_regions(self, containers, rects):
        """Rectangles of .nhwp pictures from only the tiles they touch (nhw_dec_regions): containers a list of containers (bytes), rects a
        sequence of (container index, x, y, w, h) in the coordinates of decode_pictures' arrays -> a list of numpy uint8 [h, w, 3], region i
        equal to decode_pictures(containers)[container][y:y + h, x:x + w].  Raises on any status that is not NHW_OK."""
        return self._regions_host(containers, rects, "decode_regions", lambda *a: self.lib.nhw_dec_regions(self.h, *a))

    def decode_regions_device(self, containers, rects, out=None):
        """decode_regions with the pixels left on the device (nhw_dec_regions_to_device): -> a list of uint8 CUDA tensors [h, w, 3] on this
        decoder's device.  out: a list of preallocated tensors, one a rect, with strides (pitch >= 3 w, 3, 1) -- views into an [n, h, w, 3]
        batch tensor work --, which are filled and returned.  The work is ordered after torch's current stream and complete on return."""
        return self._regions_device(containers, rects, out, "decode_regions_device", lambda *a: self.lib.nhw_dec_regions_to_device(self.h, *a))

    def decode_windows(self, containers, rects, scale=1):
        """Rectangles of .nhwp pictures at scale 1, 2 or 4, every tile decoded once (nhw_dec_windows): containers and
        rects as for decode_regions, the rectangles in the coordinates of decode_pictures_scaled's arrays at that scale -> a list of numpy uint8
        [h, w, 3], window i equal to decode_pictures_scaled(containers, scale)[container][y:y + h, x:x + w].  The tiles of the call are the union
        of the windows' selections: a tile that several windows select is uploaded and decoded once (region_stats).  Raises on any status that
        is not NHW_OK."""
        scale = _scale(scale, "decode_windows")
        return self._regions_host(containers, rects, "decode_windows", lambda *a: self.lib.nhw_dec_windows(self.h, *a[:5], scale, *a[5:]))

    def decode_windows_device(self, containers, rects, scale=1, out=None):
        """decode_windows with the pixels left on the device (nhw_dec_windows_to_device); out and the stream ordering as for
        decode_regions_device."""
        scale = _scale(scale, "decode_windows_device")
        return self._regions_device(containers, rects, out, "decode_windows_device",
                                    lambda *a: self.lib.nhw_dec_windows_to_device(self.h, *a[:5], scale, *a[5:]))

    def decode_windows_grey(self, containers, rects, scale=1):
        """decode_windows as grey (nhw_dec_windows_grey): the luma alone through the grey table of each tile file's
        quality, one byte a pixel -> a list of numpy uint8 [h, w], window i equal to decode_pictures_grey(containers, scale)[container][y:y + h,
        x:x + w].  The tiles, statuses and region_stats are decode_windows' own."""
        scale = _scale(scale, "decode_windows_grey")
        return self._regions_host(containers, rects, "decode_windows_grey", lambda *a: self.lib.nhw_dec_windows_grey(self.h, *a[:5], scale, *a[5:]), channels=1)

    def decode_windows_grey_device(self, containers, rects, scale=1, out=None):
        """decode_windows_grey with the pixels left on the device (nhw_dec_windows_grey_to_device): -> a list of uint8 CUDA tensors [h, w];
        out: preallocated tensors with strides (pitch >= w, 1).  The stream ordering is decode_regions_device's."""
        scale = _scale(scale, "decode_windows_grey_device")
        return self._regions_device(containers, rects, out, "decode_windows_grey_device",
                                    lambda *a: self.lib.nhw_dec_windows_grey_to_device(self.h, *a[:5], scale, *a[5:]), channels=1)

    def decode_pictures_grey(self, containers, scale=1):
        """Whole .nhwp pictures as grey at scale 1, 2 or 4 -> a list of numpy uint8 [ceil(H / scale), ceil(W / scale)]: decode_windows_grey
        with the window that is all of each picture."""
        scale = _scale(scale, "decode_pictures_grey")
        if not isinstance(containers, (list, tuple)) or len(containers) < 1:
            raise NhwError("decode_pictures_grey wants a non-empty list of containers")
        return self.decode_windows_grey(containers, [(i, 0, 0) + scaled_size(*picture_info(c), scale) for i, c in enumerate(containers)], scale)

    def decode_crops_grey_device(self, containers, crops, size, fmt, flips=None, scale=None, out=None, filter="two_tap", colours=None, tones=None):
        """decode_crops_device as grey (nhw_dec_crops_grey_to_device): fmt a TensorFormat of channels "GREY" -> (tensor
        [n, 1, out_h, out_w] or [n, out_h, out_w, 1] of fmt.dtype, the list of the scales used).  The scales and windows are chosen as there,
        the filters and their limits are the same, and so are the tiles and the statuses; out: at least n * out_h * out_w elements.
        colours: None, or one pair (gain, offset) a crop (nhw_dec_crops_mapped_to_device under a grey format).
        tones: None, or one tone table uint8 [256] a crop (nhw_dec_crops_toned_to_device, section 25)."""
        return self._crops_to_batch("decode_crops_grey_device", 1, containers, crops, size, fmt, flips, scale, out, filter, colours, tones)

    def decode_crops_device(self, containers, crops, size, fmt, flips=None, scale=None, out=None, filter="two_tap", colours=None, tones=None):
        """RandomResizedCrop's decode (nhw_dec_crops_to_device): crops, a sequence of (container index, x, y, w, h), each
        resampled to size = (out_h, out_w), mirrored left-right where flips[i] is true, and stored under fmt -> (tensor [n, 3, out_h, out_w]
        or [n, out_h, out_w, 3] of fmt.dtype on this decoder's device, the list of the scales used).  With a scale (1, 2 or 4) the crops
        are windows at that scale, as for decode_windows, and go down in one call.  With scale=None they are rectangles of the full-resolution
        pictures: crop i is decoded at crop_scale(w, h, out_w, out_h), as the window crop_window(x, y, w, h, that scale), and the crops of
        one scale go down together -- three calls at the most, each decoding the union of its windows' tiles once.  out: a contiguous tensor of
        fmt.dtype with at least n * 3 * out_h * out_w elements on this device, which is filled.  filter="area" resizes the windows under the area
        rule (nhw_dec_crops_to_device_filter): the scales and windows are chosen as before, and a window more than
        AREA_MAX_REDUCTION times the output along a side is refused before any call; filter="cubic" resizes them under the cubic rule
        (nhw_dec_crops_to_device_resample, section 20) with the limit CUBIC_MAX_REDUCTION.  Raises on any status that is not NHW_OK.  The
        work is ordered after torch's current stream and complete on return; region_stats speaks of the last of the calls.  colours: None, or
        one colour map a crop (nhw_dec_crops_mapped_to_device), as resize_to_tensor_device takes them: ColorJitter,
        RandomGrayscale, a channel mix or an inversion of each sample in the resampler's store.  tones: None, or one tone table a crop, uint8
        [3, 256] on R, G, B as the tone_* builders make it (nhw_dec_crops_toned_to_device, section 25): Posterize, Solarize, a gamma or any
        curve of each sample, applied behind the map; colours and tones combine."""
        return self._crops_to_batch("decode_crops_device", 3, containers, crops, size, fmt, flips, scale, out, filter, colours, tones)

    def _crops_to_batch(self, what, channels, containers, crops, size, fmt, flips, scale, out, filter, colours=None, tones=None):
        """decode_crops_device (channels=3) and decode_crops_grey_device (1)"""
        import numpy as np
        _filter(filter, what)
        fmt = _tensor_format(fmt, what, grey=channels == 1)
        out_h, out_w = _crop_size(size, what)
        if scale is not None:
            scale = _scale(scale, what)
        maps = tabs = None
        if colours is not None or tones is not None:
            if not isinstance(crops, (list, tuple, np.ndarray)):
                raise NhwError(f"{what}: `crops` must be a sequence, one colour map{'' if tones is None else ' or tone table'} a crop")
            maps = _colour_table(colours, len(crops), what, channels) if colours is not None else None
            tabs = _host_tones(tones, len(crops), what, channels) if tones is not None else None
        blob, offs, table = self._region_args(containers, crops, what)
        n = len(table)
        flags = _crop_flips(flips, n, what)
        if scale is None:
            x, y, w, h = (table[k].astype(np.int64) for k in ("x", "y", "width", "height"))
            if not (w.all() and h.all()):
                raise NhwError(f"{what}: crop {int(np.flatnonzero((w == 0) | (h == 0))[0])} is empty")
            sc = np.where((4 * out_w <= w) & (4 * out_h <= h), 4, np.where((2 * out_w <= w) & (2 * out_h <= h), 2, 1))   # crop_scale and crop_window, on arrays
            table["x"], table["y"] = x // sc, y // sc
            table["width"], table["height"] = -(-(x + w) // sc) - x // sc, -(-(y + h) // sc) - y // sc
            scales = sc.tolist()
        else:
            scales = [scale] * n
        if filter in _LIMITS:
            for i, r in enumerate(table):
                _filter_limit(filter, int(r["width"]), int(r["height"]), out_w, out_h, what, f"the window of crop {i}")
        call, tables = _sample_entry(self.lib, "crops", channels, maps, tabs)
        return self._rects_to_batch(what, blob, offs, len(containers), table, flags, scales, out_w, out_h, fmt, out,
                                    lambda *args: call(*args, RESAMPLERS[filter]), channels, tables), scales

    def _rects_to_batch(self, what, blob, offs, n_containers, table, extra, scales, out_w, out_h, fmt, out, call, channels=3, tables=()):
        """the device side of decode_crops_device and decode_warps_device: the checked batch tensor (`out`, or a new one), and per scale one
        call(handle, blob, offsets, n containers, the scale's rects, their count, scale, out_w, out_h, format, the scale's rows of `extra` --
        the flag bytes or the nhw_warp table, or None --, the scale's rows of each of `tables` -- the table arguments of _sample_entry: nothing, the
        nhw_colour_map table of a mapped call, or the maps (or None, a null pointer) and the uint8 [n, 768] table of a toned call --, the tensors' addresses,
        statuses) -> rc.  Raises on any status that is not NHW_OK"""
        import numpy as np
        t = self.torch
        n = len(table)
        dev = t.device("cuda", self.device)
        shape = (n,) + fmt.shape(out_h, out_w)
        per = channels * out_h * out_w
        if out is None:
            out = t.empty(shape, dtype=fmt.dtype, device=dev)
        elif not (isinstance(out, t.Tensor) and out.is_cuda and out.device == dev and out.dtype == fmt.dtype and out.is_contiguous() and out.numel() >= n * per):
            raise NhwError(f"{what}: `out` must be a contiguous {fmt.dtype} tensor of at least {n}*{per} elements on {dev}")
        addr = np.uint64(out.data_ptr()) + np.arange(n, dtype=np.uint64) * np.uint64(per * out.element_size())
        status = np.zeros(n, np.int32)
        c = fmt.c_struct()
        t.cuda.current_stream(dev).synchronize()                     # the calls run on the handle's own stream and wait for it
        for s in sorted(set(scales)):
            idx = np.flatnonzero(np.array(scales) == s)
            sub, a, st = np.ascontiguousarray(table[idx]), np.ascontiguousarray(addr[idx]), np.empty(len(idx), np.int32)
            x = np.ascontiguousarray(extra[idx]) if extra is not None else None
            mp = [np.ascontiguousarray(m[idx]) if m is not None else None for m in tables]
            self._chk(call(self.h, blob.ctypes.data, offs.ctypes.data, n_containers, sub.ctypes.data, len(idx), s, out_w, out_h,
                           ctypes.byref(c), x.ctypes.data if x is not None else None, *(m.ctypes.data if m is not None else None for m in mp), a.ctypes.data, st.ctypes.data))
            status[idx] = st
        self._region_raise(status)
        return out if tuple(out.shape) == shape else out.reshape(-1)[:n * per].view(shape)

    def decode_warps_grey_device(self, containers, which, matrices, size, fmt, fill=0, border="fill", scale=None, out=None, colours=None, tones=None):
        """decode_warps_device as grey (nhw_dec_warps_grey_to_device): fmt a TensorFormat of channels "GREY", fill one
        byte -> (tensor [n, 1, out_h, out_w] or [n, out_h, out_w, 1] of fmt.dtype, the list of the scales used).  The scales and windows are
        chosen as there.  colours: None, or one pair (gain, offset) a warp; tones: None, or one table uint8 [256] a warp."""
        return self._warps_to_batch("decode_warps_grey_device", 1, containers, which, matrices, size, fmt, fill, border, scale, out, colours, tones)

    def decode_warps_device(self, containers, which, matrices, size, fmt, fill=(0, 0, 0), border="fill", scale=None, out=None, colours=None, tones=None):
        """RandomAffine's / RandomRotation's decode (nhw_dec_warps_to_device): warp i samples the picture of container
        which[i] along the grid of matrices[i] -- a 2 x 3 matrix of floats as warp_fixed takes it, in FULL-resolution picture coordinates
        (crop_warp makes one from a rectangle, an angle and a flip) -- into size = (out_h, out_w), and is stored under fmt -> (tensor [n, 3,
        out_h, out_w] or [n, out_h, out_w, 3] of fmt.dtype on this decoder's device, the list of the scales used).  With scale=None warp i is
        decoded at warp_scale(matrices[i]) and the warps of one scale go down together, three calls at the most; with a scale (1, 2 or 4),
        one call at that scale.  Each warp's window is warp_window's -- only the tiles it touches are uploaded and decoded, each once a call
        -- and the result is, byte for byte, the warp of the whole picture decoded at that scale under warp_fixed(matrix / scale).  A tap
        outside the picture takes fill = (B, G, R), or with border="replicate" the nearest edge pixel.  out: as for decode_crops_device.
        Raises on any status that is not NHW_OK.  The work is ordered after torch's current stream and complete on return; region_stats
        speaks of the last of the calls.  colours: None, or one colour map a warp (nhw_dec_warps_mapped_to_device), as
        decode_crops_device takes them; the border colour is mapped like any other pixel.  tones: None, or one tone table a warp
        (nhw_dec_warps_toned_to_device, section 25), as decode_crops_device takes them; the border colour goes through the table too."""
        return self._warps_to_batch("decode_warps_device", 3, containers, which, matrices, size, fmt, fill, border, scale, out, colours, tones)

    def _warps_to_batch(self, what, channels, containers, which, matrices, size, fmt, fill, border, scale, out, colours=None, tones=None):
        """decode_warps_device (channels=3) and decode_warps_grey_device (1)"""
        import numpy as np
        fmt = _tensor_format(fmt, what, grey=channels == 1)
        out_h, out_w = _crop_size(size, what)
        fill, flags = _warp_border(fill, border, what, channels)
        if scale is not None:
            scale = _scale(scale, what)
        if not isinstance(containers, (list, tuple)) or len(containers) < 1:
            raise NhwError(f"{what} wants a non-empty list of containers")
        if not isinstance(which, (list, tuple, np.ndarray)) or not isinstance(matrices, (list, tuple, np.ndarray)) or len(which) < 1 or len(which) != len(matrices):
            raise NhwError(f"{what}: `which` and `matrices` must be non-empty and of the same length: one container index and one matrix a warp")
        n = len(which)
        maps = _colour_table(colours, n, what, channels) if colours is not None else None
        tabs = _host_tones(tones, n, what, channels) if tones is not None else None
        for i, ci in enumerate(which):
            if isinstance(ci, bool) or not isinstance(ci, numbers.Integral) or not 0 <= ci < len(containers):
                raise NhwError(f"{what}: which[{i}] must be a container index of 0 .. {len(containers) - 1}, got {ci!r}")
        mats = [_warp_matrix(m, f"{what}: matrix {i}") for i, m in enumerate(matrices)]
        scales = [warp_scale(m) for m in mats] if scale is None else [scale] * n
        sizes, rects, fixed = {}, [], []
        for i, (ci, m, s) in enumerate(zip(which, mats, scales)):
            if ci not in sizes:
                sizes[ci] = picture_info(containers[ci])
            win, fx = warp_window(m, (out_h, out_w), *sizes[ci], s)
            rects.append((int(ci),) + win)
            fixed.append(fx)
        blob, offs, table = self._region_args(containers, rects, what)
        call, tables = _sample_entry(self.lib, "warps", channels, maps, tabs)
        return self._rects_to_batch(what, blob, offs, len(containers), table, _warp_table(fixed, fill, flags), scales, out_w, out_h, fmt, out, call, channels, tables), scales

    def region_stats(self):
        """(tiles handed to the decoder, tile-file bytes uploaded) of this handle's last region or window call (nhw_dec_last_region_stats);
        after a window call the tiles are the unique ones"""
        a, b = ctypes.c_uint64(), ctypes.c_uint64()
        self._chk(self.lib.nhw_dec_last_region_stats(self.h, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def decode(self, files):
        """files: list of .nhw byte strings -> (uint8 [n,512,512,3] in nhw-dec's output byte order, quality list)."""
        import numpy as np
        n = len(files)
        offs = np.zeros(n + 1, np.uint64)
        offs[1:] = np.cumsum([len(f) for f in files])
        blob = np.frombuffer(b"".join(files), np.uint8)
        out = np.empty((n, 512, 512, 3), np.uint8)
        status = np.empty(n, np.int32)
        quality = np.empty(n, np.int32)
        self._chk(self.lib.nhw_dec_batch(self.h, blob.ctypes.data, offs.ctypes.data, n, out.ctypes.data, status.ctypes.data, quality.ctypes.data))
        if (status != 0).any():
            raise NhwError(f"per-file status {status.tolist()}")
        return out, quality.tolist()
