"""ctypes binding of libst_amd.so (C ABI declared in include/st_amd.h).

PyTorch is used for device memory and streams only: every call below hands raw ``data_ptr()``s and
the current HIP stream to the library.  There is NO fallback: if the library is missing, was not
built for gfx950, or no GPU is visible, loading fails with an explicit error.
"""

import ctypes
import os

import torch

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# in-tree (repo checkout, `pip install -e`): style-transfer-pytorch_amd/lib/; installed wheel / non-editable install:
# setup.py's build step copies the library INTO the package (style_transfer/lib/)
_LIB_CANDIDATES = (os.path.join(_PKG_ROOT, 'lib', 'libst_amd.so'),
                   os.path.join(os.path.dirname(os.path.abspath(__file__)), 'lib', 'libst_amd.so'))
LIB_PATH = next((c for c in _LIB_CANDIDATES if os.path.exists(c)), _LIB_CANDIDATES[0])

_c_float_p = ctypes.c_void_p      # device pointers travel as integers
# features indices the trunk keeps: the 13 ReLU outputs and the 4 pool outputs (st_plan_feature)
TAPS = (1, 3, 4, 6, 8, 9, 11, 13, 15, 17, 18, 20, 22, 24, 26, 27, 29)
DEFAULT_CONTENT_LAYERS, DEFAULT_STYLE_LAYERS = (22,), (1, 6, 11, 20, 29)
# the loss kind of each list (st_plan_set_loss_kinds), by the library's code: ContentLossMSE / ContentLoss, StyleLossW2 / StyleLoss
CONTENT_LOSSES, STYLE_LOSSES = ('mse', 'scaled_mse'), ('w2', 'gram')
# what a nearest head is matched on (st_plan_set_nearest_metric's codes 0, 1, 2; include/st_amd.h)
NEAREST_METRICS = ('l2', 'cosine', 'centered_cosine')
_lib = None


class HipLibraryError(RuntimeError):
    pass


class Exchange(ctypes.Structure):
    """st_exchange (include/st_amd.h): what must be exchanged between two closure phases."""
    _fields_ = [('kind', ctypes.c_int), ('count', ctypes.c_longlong), ('send_up', ctypes.c_void_p),
                ('send_down', ctypes.c_void_p), ('recv_up', ctypes.c_void_p), ('recv_down', ctypes.c_void_p),
                ('buffer', ctypes.c_void_p), ('root', ctypes.c_int), ('channel', ctypes.c_int),
                ('stream', ctypes.c_void_p)]


def _declare(lib):
    vp, i32, i64, f64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_longlong, ctypes.c_double, ctypes.c_float
    pp = ctypes.POINTER(ctypes.c_void_p)
    ip = ctypes.POINTER(ctypes.c_int)
    sig = {
        'st_last_error': (ctypes.c_char_p, []),
        'st_abi_version': (i32, []),
        'st_compiled_arch': (ctypes.c_char_p, []),
        'st_max_pixels': (ctypes.c_longlong, []),
        'st_has_experiments': (i32, []),
        'st_env_switches': (i32, [ctypes.POINTER(ctypes.c_char_p), i32]),
        'st_set_option': (i32, [ctypes.c_char_p, i32, i32]),
        'st_net_create': (i32, [pp, pp, pp, i32]),
        'st_net_create_ex': (i32, [pp, pp, pp, i32, i32]),
        'st_net_destroy': (i32, [vp]),
        'st_net_wide_layers': (i32, [vp, ip, ip]),
        'st_net_mark_wide': (i32, [vp, ip, ip]),
        'st_plan_create': (i32, [pp, vp, i32, i32]),
        'st_plan_range_guard': (i32, [vp, vp, ip, ip, vp]),
        'st_plan_destroy': (i32, [vp]),
        'st_plan_device_bytes': (i64, [vp]),
        'st_plan_forward': (i32, [vp, vp, i32, vp]),
        'st_plan_feature': (i32, [vp, i32, pp, ip, ip, ip]),
        'st_plan_backward': (i32, [vp, i32, ip, pp, vp, vp]),
        'st_plan_moments': (i32, [vp, i32, vp, vp, vp]),
        'st_plan_set_style_mask': (i32, [vp, vp, vp]),
        'st_plan_style_mask': (i32, [vp, i32, pp, ip, ip, ctypes.POINTER(f64)]),
        'st_plan_set_style_regions': (i32, [vp, i32, pp, vp]),
        'st_plan_style_region': (i32, [vp, i32, i32, pp, ip, ip, ctypes.POINTER(f64)]),
        'st_plan_set_region_style_target': (i32, [vp, i32, i32, vp, vp, vp]),
        'st_plan_set_region_weights': (i32, [vp, ctypes.POINTER(f32)]),
        'st_plan_region_terms': (i32, [vp, pp, ip, ip]),
        'st_plan_set_content_mask': (i32, [vp, vp, vp]),
        'st_plan_content_mask': (i32, [vp, i32, pp, ip, ip]),
        'st_plan_set_tv_mask': (i32, [vp, vp, vp]),
        'st_plan_tv_mask': (i32, [vp, pp, ip, ip]),
        'st_plan_set_laplacian': (i32, [vp, vp, i32, ip, f32, vp]),
        'st_plan_laplacian': (i32, [vp, i32, pp, ip, ip]),
        'st_plan_laplacian_terms': (i32, [vp, pp, ip]),
        'st_plan_set_content_target': (i32, [vp, vp, vp]),
        'st_plan_set_style_target': (i32, [vp, i32, vp, vp, vp]),
        'st_plan_set_loss_weights': (i32, [vp, f32, ctypes.POINTER(f32), f32]),
        'st_plan_set_taps': (i32, [vp, i32, ip, i32, ip]),
        'st_plan_set_tap_weights': (i32, [vp, ctypes.POINTER(f32), ctypes.POINTER(f32), f32]),
        'st_plan_set_loss_kinds': (i32, [vp, i32, i32]),
        'st_plan_loss_kinds': (i32, [vp, ip, ip]),
        'st_plan_set_layer_loss_kinds': (i32, [vp, ip, ip]),
        'st_plan_layer_loss_kinds': (i32, [vp, ip, ip]),
        'st_plan_set_loss_eps': (i32, [vp, ctypes.POINTER(f32), ctypes.POINTER(f32)]),
        'st_plan_loss_eps': (i32, [vp, ctypes.POINTER(f32), ctypes.POINTER(f32)]),
        'st_plan_set_w2_diagonal': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_w2_diagonal': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_set_w2_marginal': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_w2_marginal': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_set_style_quantiles': (i32, [vp, i32, vp, i64, vp]),
        'st_plan_style_quantiles': (i32, [vp, i32, pp, ip, ctypes.POINTER(i64)]),
        'st_plan_set_style_nearest': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_style_nearest': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_set_style_vectors': (i32, [vp, i32, vp, i64, vp]),
        'st_plan_nearest_indices': (i32, [vp, i32, pp, ctypes.POINTER(i64)]),
        'st_plan_set_nearest_metric': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_nearest_metric': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_set_style_sliced': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_style_sliced': (i32, [vp, ctypes.POINTER(i32)]),
        'st_plan_set_sliced_options': (i32, [vp, i32, i32, i32]),
        'st_plan_set_sliced_seed': (i32, [vp, ctypes.c_ulonglong]),
        'st_plan_set_style_sliced_vectors': (i32, [vp, i32, i32, pp, ctypes.POINTER(i64), ctypes.POINTER(f32), vp]),
        'st_plan_sliced_directions': (i32, [vp, i32, pp, ip, ip, ctypes.POINTER(ctypes.c_ulonglong)]),
        'st_plan_sliced_target': (i32, [vp, i32, pp, ip, ctypes.POINTER(i64)]),
        'st_plan_set_content_target_at': (i32, [vp, i32, vp, vp]),
        'st_plan_term_losses': (i32, [vp, pp, ip]),
        'st_plan_loss_and_grad': (i32, [vp, vp, vp, vp, vp]),
        'st_plan_step': (i32, [vp, vp, vp, vp, vp, i64, f64, f64, f64, f64, f64, vp, vp]),
        'st_plan_apply_update': (i32, [vp, vp, vp, vp, vp, vp, i64, f64, f64, f64, f64, f64, vp]),
        'st_lbfgs_state_bytes': (i64, [i64]),
        'st_lbfgs_reset': (i32, [vp, i64, vp]),
        'st_lbfgs_update': (i32, [vp, i64, vp, vp, vp, f64, vp]),
        'st_plan_lbfgs_step': (i32, [vp, vp, vp, vp, f64, vp, vp]),
        'st_lbfgs_info': (i32, [vp, i64, ip, ip, ip, ip, ctypes.POINTER(f64), ctypes.POINTER(f64), vp]),
        'st_qn_strip_state_bytes': (i64, [i64, i32]),
        'st_qn_strip_dots': (i32, [vp, i64, i32, i32, vp, ctypes.POINTER(Exchange), vp]),
        'st_qn_strip_apply': (i32, [vp, i64, i32, vp, vp, vp, f64, vp]),
        'st_plan_qn_strip_step': (i32, [vp, vp, vp, vp, vp, vp, f64, vp]),
        'st_plan_create_strip': (i32, [pp, vp, i32, i32, i32, i32]),
        'st_plan_closure_begin': (i32, [vp, vp, vp]),
        'st_plan_set_rank': (i32, [vp, i32, i32]),
        'st_plan_closure_next': (i32, [vp, ctypes.POINTER(Exchange), vp]),
        'st_fabric_unique_id': (i32, [ctypes.c_char_p]),
        'st_fabric_create': (i32, [pp, ctypes.c_char_p, ctypes.c_char_p, i32, i32, i32]),
        'st_fabric_destroy': (i32, [vp]),
        'st_fabric_abort': (i32, [vp]),
        'st_fabric_selftest': (i32, [vp, vp, i32]),
        'st_plan_closure_run': (i32, [vp, vp, vp]),
        'st_plan_losses': (i32, [vp, pp]),
        'st_plan_debug_read': (i32, [vp, i32, ctypes.POINTER(f32), i32]),
        'st_plan_forward_begin': (i32, [vp, vp, i32]),
        'st_plan_moment_sums': (i32, [vp, i32, vp, vp]),
        'st_plan_set_graph': (i32, [vp, i32]),
        'st_plan_profile_enable': (i32, [vp, i32]),
        'st_plan_profile_read': (i32, [vp, ctypes.POINTER(i64), ctypes.POINTER(f64), ctypes.POINTER(f64)]),
        'st_plan_profile_read_hbm': (i32, [vp, i32, ctypes.POINTER(i64), ctypes.POINTER(f64), ctypes.POINTER(f64)]),
        'st_op_sqrtm_ns': (i32, [vp, vp, i32, vp]),
        'st_op_sqrtm_ns_backward': (i32, [vp, vp, vp, i32, vp]),
        'st_op_sqrtm_ns_backward_diag': (i32, [vp, f32, vp, i32, vp]),
        'st_op_tv_loss': (i32, [vp, i32, i32, vp, vp, vp]),
        'st_op_sqrtm_time': (i32, [i32, i32, ctypes.POINTER(f64), ctypes.POINTER(f64), vp]),
        'st_op_mfma_rate': (i32, [i32, i32, i32, i32, ctypes.POINTER(f64), ctypes.POINTER(f64), vp]),
        'st_op_mfma_valu_rate': (i32, [i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(f64), ctypes.POINTER(f64),
                                       ctypes.POINTER(f64), vp]),
        'st_op_grid_barrier_time': (i32, [i32, i32, i32, i32, ctypes.POINTER(f64), ip, vp]),
        'st_op_winograd_consumer_rate': (i32, [i32, i32, ctypes.POINTER(f64), vp]),
        'st_op_conv3x3_time': (i32, [i32, i32, i32, i32, i32, i32, i32, ctypes.POINTER(f64), vp]),
        'st_op_conv3x3': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, vp]),
        'st_op_conv3x3_dgrad': (i32, [vp, vp, vp, vp, i32, i32, i32, i32, i32, vp]),
        'st_op_conv3x3_strip': (i32, [vp, vp, i32, i32, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, vp]),
        'st_op_conv3x3_strip_ex': (i32, [vp, vp, i32, i32, vp, vp, vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp]),
        'st_op_conv1x1': (i32, [vp, vp, vp, vp, i32, i32, i64, i32, vp]),
        'st_op_pool2x2': (i32, [vp, vp, i32, i32, i32, i32, vp]),
        'st_op_pool2x2_backward': (i32, [vp, vp, vp, i32, i32, i32, i32, vp]),
        'st_head_create': (i32, [pp, i32, i32, i32, i32, i32]),
        'st_head_destroy': (i32, [vp]),
        'st_head_device_bytes': (i64, [vp]),
        'st_head_state_floats': (i64, [vp]),
        'st_head_moments': (i32, [vp, vp, vp, vp, vp]),
        'st_op_gram_split_plan': (i32, [i32, i64, i32, ip, ctypes.POINTER(i64), ip]),
        'st_head_forward': (i32, [vp, vp, vp, vp, vp, vp, f32, vp, vp, vp]),
        'st_head_backward': (i32, [vp, vp, vp, vp, vp, vp]),
        'st_op_reduce_scratch_floats': (i64, []),
        'st_op_mse_loss': (i32, [vp, vp, i64, vp, vp, vp]),
        'st_op_mse_loss_backward': (i32, [vp, vp, i64, vp, vp, vp]),
        'st_op_scaled_mse_loss': (i32, [vp, vp, i64, f32, vp, vp, vp, vp]),
        'st_op_scaled_mse_loss_backward': (i32, [vp, vp, i64, vp, vp, vp, vp]),
        'st_op_channel_stats_scratch_floats': (i64, [i32, i64]),
        'st_op_channel_moments': (i32, [vp, i32, i64, vp, vp, vp, vp]),
        'st_op_w2_diag_loss': (i32, [vp, i32, i64, vp, vp, f32, vp, vp, vp, vp]),
        'st_op_w2_diag_loss_backward': (i32, [vp, i32, i64, vp, vp, vp, vp]),
        'st_op_sort_chunk': (i32, []),
        'st_op_sort_scratch_bytes': (i64, [i32, i64]),
        'st_op_channel_sort': (i32, [vp, i32, i64, vp, vp, vp, vp]),
        'st_op_resample_quantiles': (i32, [vp, i32, i64, i64, vp, vp]),
        'st_op_w2_marginal_loss': (i32, [vp, i32, i64, vp, vp, vp, vp, vp]),
        'st_op_w2_marginal_loss_backward': (i32, [vp, i64, vp, vp, vp]),
        'st_op_nearest_k_chunk': (i32, []),
        'st_op_nearest_pixel_tile': (i32, []),
        'st_op_nearest_k_tile': (i32, []),
        'st_op_nearest_splits': (i32, [i64, i64]),
        'st_op_nearest_prepared_floats': (i64, [i32, i64]),
        'st_op_nearest_scratch_floats': (i64, [i32, i64, i64]),
        'st_op_nearest_prepare': (i32, [vp, i32, i64, vp, vp]),
        'st_op_nearest_search': (i32, [vp, i32, i64, vp, i64, vp, vp, vp, vp]),
        'st_op_nearest_loss': (i32, [vp, i32, i64, vp, i64, vp, vp, vp, vp, vp]),
        'st_op_nearest_loss_backward': (i32, [vp, i64, vp, vp, vp]),
        'st_op_nearest_cosine_prepared_floats': (i64, [i32, i64]),
        'st_op_nearest_cosine_scratch_floats': (i64, [i32, i64, i64]),
        'st_op_nearest_cosine_prepare': (i32, [vp, i32, i64, i32, vp, vp]),
        'st_op_nearest_cosine_loss': (i32, [vp, i32, i64, vp, i64, vp, vp, vp, vp, vp]),
        'st_op_sliced_directions': (i32, [ctypes.c_ulonglong, i32, ctypes.c_ulonglong, i32, i32, vp, vp, vp]),
        'st_op_sliced_scratch_bytes': (i64, [i32, i32, i64]),
        'st_op_sliced_target': (i32, [vp, i32, i64, vp, vp, i32, i64, vp, vp, i32, f32, vp]),
        'st_op_sliced_project': (i32, [vp, i32, i64, vp, vp, i32, vp, vp, vp]),
        'st_op_sliced_loss': (i32, [vp, i32, i64, vp, vp, i32, vp, vp, vp, vp, vp]),
        'st_op_sliced_loss_backward': (i32, [vp, i64, vp, vp, vp]),
        'st_op_tv_value': (i32, [vp, i32, i32, vp, vp, vp]),
        'st_op_tv_loss_backward': (i32, [vp, i32, i32, vp, vp, vp]),
        'st_op_mse_term': (i32, [vp, vp, i64, f32, vp, vp, vp, vp, vp]),
        'st_op_tv_term': (i32, [vp, i32, i32, f32, vp, vp, vp, vp, vp]),
        'st_op_laplacian_scratch_floats': (i64, [i32, i32, i32, i32]),
        'st_op_laplacian_target': (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
        'st_op_laplacian_value': (i32, [vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]),
        'st_op_laplacian_backward': (i32, [vp, i32, i32, i32, i32, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)       # AttributeError here = header and library disagree
        fn.restype = res
        fn.argtypes = args
    return sig


EXPORTED_SYMBOLS = None


def load_library(require_gpu=True):
    """Load libst_amd.so.  ``require_gpu=False`` is only for the CPU-side symbol/ABI check."""
    global _lib, EXPORTED_SYMBOLS
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise HipLibraryError(
                f'{LIB_PATH} not found: build it with `python style-transfer-pytorch_amd/build.py` '
                '(needs hipcc, targets gfx950).  This package has no CPU or PyTorch fallback.')
        lib = ctypes.CDLL(LIB_PATH)
        EXPORTED_SYMBOLS = sorted(_declare(lib))
        if lib.st_abi_version() != 2:
            raise HipLibraryError('libst_amd.so ABI version mismatch')
        _lib = lib
    if require_gpu and not torch.cuda.is_available():
        raise HipLibraryError('no HIP device visible: the MI355X hot path cannot run (no CPU fallback)')
    return _lib


def max_pixels():
    """The most pixels (H * W, or npix) one image, strip, tap or feature map may hold at any entry point of the library
    (st_max_pixels: 2^24 - 1; include/st_amd.h, "Size limit")."""
    return int(load_library(require_gpu=False).st_max_pixels())


def has_experiments():
    """True when libst_amd.so was built with ``build.py --experiments`` (Winograd conv, persistent NS chain kernel, ...)."""
    return bool(load_library(require_gpu=False).st_has_experiments())


def env_switches():
    """The ST_* switches a default build reads from the environment (everything else: ``set_option`` / ``options``)."""
    lib = load_library(require_gpu=False)
    names = (ctypes.c_char_p * 64)()
    n = lib.st_env_switches(names, 64)
    return [names[i].decode() for i in range(n)]


_overrides = {}      # this process's current st_set_option overrides (the library has no getter)


def set_option(name, value=None):
    """Override (or, with value=None, clear) one of the library's ST_* switches for this process."""
    lib = load_library(require_gpu=False)
    _check(lib.st_set_option(name.encode(), int(value or 0), 1 if value is None else 0))
    if value is None:
        _overrides.pop(name, None)
    else:
        _overrides[name] = int(value)


class options:
    """Context manager: ``with options(ST_CONV_PC=0): ...`` runs the block with the switches overridden and puts the
    PREVIOUS overrides back afterwards (nested / outer overrides of the same switch survive)."""

    def __init__(self, **kv):
        self.kv = kv
        self.saved = {}

    def __enter__(self):
        self.saved = {k: _overrides.get(k) for k in self.kv}
        for k, v in self.kv.items():
            set_option(k, v)

    def __exit__(self, *exc):
        for k, prev in self.saved.items():
            set_option(k, prev)


def _check(rc):
    if rc != 0:
        raise HipLibraryError(load_library(False).st_last_error().decode('utf-8', 'replace'))


def _ptr(t):
    if t is None:
        return None
    assert t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(), 'expected a contiguous fp32 HIP tensor'
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Net:
    """Frozen VGG-19 trunk on one device (st_net)."""

    PRECISIONS = {'fp32': 0, 'bf16x3': 2, 'bf16x6': 3, 'fp16x3': 4}

    def __init__(self, params, pooling, device, precision='fp32'):
        self.lib = load_library()
        self.device = torch.device(device)
        self.pooling = pooling
        self.precision = precision
        with torch.cuda.device(self.device):
            dev = [(w.to(self.device, torch.float32).contiguous(), b.to(self.device, torch.float32).contiguous())
                   for w, b in params]
            wa = (ctypes.c_void_p * 13)(*[w.data_ptr() for w, _ in dev])
            ba = (ctypes.c_void_p * 13)(*[b.data_ptr() for _, b in dev])
            h = ctypes.c_void_p()
            torch.cuda.synchronize(self.device)
            _check(self.lib.st_net_create_ex(ctypes.byref(h), wa, ba, {'max': 0, 'average': 1, 'l2': 2}[pooling],
                                             self.PRECISIONS[precision]))
        self.handle = h

    def wide_layers(self):
        """([13 ints], [13 ints]): convolutions whose forward / data gradient the fp16x3 dynamic-range guard moved to
        bf16x6 (st_net_wide_layers)."""
        fwd, bwd = (ctypes.c_int * 13)(), (ctypes.c_int * 13)()
        _check(self.lib.st_net_wide_layers(self.handle, fwd, bwd))
        return list(fwd), list(bwd)

    def mark_wide(self, forward13, backward13):
        """Add layers to the bf16x6 set (st_net_mark_wide): the union of the ranks' range-guard verdicts in a sharded run."""
        fwd, bwd = (ctypes.c_int * 13)(*[int(v) for v in forward13]), (ctypes.c_int * 13)(*[int(v) for v in backward13])
        with torch.cuda.device(self.device):
            _check(self.lib.st_net_mark_wide(self.handle, fwd, bwd))

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and self.lib is not None:
            self.lib.st_net_destroy(h)


class Plan:
    """All device buffers and kernels for one image size (st_plan)."""

    # bumped by every call that overwrites the activations (forward, loss_and_grad, step, range_guard, LBFGS.step): whoever
    # keeps a forward's taps for a later backward() compares it to know whether that forward is still the current one
    forward_count = 0
    # the configured layers (set_taps); strip plans keep the default
    content_layers, style_layers = DEFAULT_CONTENT_LAYERS, DEFAULT_STYLE_LAYERS
    # the lists' loss kinds (set_loss_kinds): the name while a list's layers agree, the tuple of names once they differ
    # (set_layer_loss_kinds); per layer: content_losses / style_losses
    content_loss, style_loss = CONTENT_LOSSES[0], STYLE_LOSSES[0]

    def __init__(self, net, height, width):
        self.lib = net.lib
        self.net = net
        self.device = net.device
        self.height, self.width = int(height), int(width)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            rc = self.lib.st_plan_create(ctypes.byref(h), net.handle, self.height, self.width)
        if rc != 0:
            msg = self.lib.st_last_error().decode()
            if 'must be at least' in msg:
                raise ValueError(msg)          # same exception type as VGGFeatures.forward (:83)
            raise HipLibraryError(msg)
        self.handle = h
        self.losses = torch.zeros(8, device=self.device, dtype=torch.float32)

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and self.lib is not None:
            self.lib.st_plan_destroy(h)

    def set_taps(self, content_layers, style_layers):
        """The layers of the closure's content / style terms (st_plan_set_taps): any of ``TAPS``, 0 to 16 per list, each once
        per list, at least one in all.  Drops every target set before and resets the weights to the lists'
        defaults (``set_loss_weights`` afterwards; only the default lists named again on a plan that has them keep
        theirs).  Anything but the default lists runs the general closure."""
        content_layers, style_layers = [int(v) for v in content_layers], [int(v) for v in style_layers]
        ca = (ctypes.c_int * max(len(content_layers), 1))(*content_layers)
        sa = (ctypes.c_int * max(len(style_layers), 1))(*style_layers)
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_taps(self.handle, len(content_layers), ca, len(style_layers), sa))
        self.content_layers, self.style_layers = content_layers, style_layers
        self._read_loss_kinds()         # (a mixed list has returned to its default kind)

    def set_loss_kinds(self, content='mse', style='w2'):
        """What the terms are, one kind per list (st_plan_set_loss_kinds): ``content`` one of ``CONTENT_LOSSES`` - 'mse'
        (ContentLossMSE) or 'scaled_mse' (ContentLoss) - and ``style`` one of ``STYLE_LOSSES`` - 'w2' (StyleLossW2) or 'gram'
        (StyleLoss on Gram matrices).  Drops every target set before; the layers and all weights stay.  Anything but the
        defaults runs the general closure; strip plans refuse it."""
        if content not in CONTENT_LOSSES:
            raise ValueError(f'content loss {content!r}: must be one of {CONTENT_LOSSES}')
        if style not in STYLE_LOSSES:
            raise ValueError(f'style loss {style!r}: must be one of {STYLE_LOSSES}')
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_loss_kinds(self.handle, CONTENT_LOSSES.index(content), STYLE_LOSSES.index(style)))
        self.content_loss, self.style_loss = content, style

    def set_layer_loss_kinds(self, content, style):
        """The same per layer (st_plan_set_layer_loss_kinds): one name of ``CONTENT_LOSSES`` per content layer and one of
        ``STYLE_LOSSES`` per style layer, in list order.  Lists whose names agree are ``set_loss_kinds``' setting; on any
        other, every head runs by its own kind in the general closure, and ``content_loss`` / ``style_loss`` become the
        tuple.  Drops every target and returns every eps to its default."""
        content, style = list(content), list(style)
        if len(content) != len(self.content_layers) or len(style) != len(self.style_layers):
            raise ValueError(f'{len(content)} content and {len(style)} style loss kinds for {len(self.content_layers)} content and '
                             f'{len(self.style_layers)} style layers: one per layer')
        for name in content:
            if name not in CONTENT_LOSSES:
                raise ValueError(f'content loss {name!r}: must be one of {CONTENT_LOSSES}')
        for name in style:
            if name not in STYLE_LOSSES:
                raise ValueError(f'style loss {name!r}: must be one of {STYLE_LOSSES}')
        ca = (ctypes.c_int * max(len(content), 1))(*[CONTENT_LOSSES.index(name) for name in content])
        sa = (ctypes.c_int * max(len(style), 1))(*[STYLE_LOSSES.index(name) for name in style])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_layer_loss_kinds(self.handle, ca, sa))
        self._read_loss_kinds()

    def set_loss_eps(self, content=None, style=None):
        """The eps of each layer's loss module (st_plan_set_loss_eps): per list None (every layer's default), a number
        (every layer) or a sequence with a number or None per layer.  The defaults are the reference's constructors': 1e-4
        for 'w2', 1e-8 for 'gram' and 'scaled_mse'; 'mse' has none.  Anything but the defaults runs the general closure;
        drops every target.  Either kinds setter and ``set_taps`` return every eps to its default: kinds first, then eps,
        then the targets."""
        arrays = []
        for given, layers, what in ((content, self.content_layers, 'content'), (style, self.style_layers, 'style')):
            if given is None or isinstance(given, (int, float)):
                given = [given] * len(layers)
            given = list(given)
            if len(given) != len(layers):
                raise ValueError(f'{len(given)} {what} eps for {len(layers)} {what} layers: one per layer')
            for v in given:
                if v is not None and not float(v) >= 0:
                    raise ValueError(f'{what} eps {v!r}: must be None or a non-negative number')
            arrays.append((ctypes.c_float * max(len(given), 1))(*[-1.0 if v is None else float(v) for v in given]))
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_loss_eps(self.handle, *arrays))

    def set_w2_diagonal(self, flags=None):
        """Restrict both covariances of a 'w2' style layer to their diagonals (st_plan_set_w2_diagonal): None or False (no
        layer), True (every layer of the list - all must be 'w2') or a sequence with one bool per style layer.  A flagged
        layer's term is ``sum (mu - mu_t)^2 + sum (sigma - sigma_t)^2`` over the channels, divided by their number: two
        memory-bound launches, no C x C work.  Any set flag runs the general closure; drops every target.  Either kinds
        setter and ``set_taps`` clear the flags: kinds, eps, then this, then the weights and targets."""
        n = len(self.style_layers)
        if flags is None or isinstance(flags, (bool, int)):
            flags = [bool(flags)] * n
        flags = list(flags)
        if len(flags) != n:
            raise ValueError(f'{len(flags)} diagonal flags for {n} style layers: one per layer')
        for v in flags:
            if v not in (0, 1, False, True):
                raise ValueError(f'diagonal flag {v!r}: must be a bool')
        fa = (ctypes.c_int * max(n, 1))(*[int(v) for v in flags])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_w2_diagonal(self.handle, fa))

    @property
    def w2_diagonal(self):
        """The diagonal flag of each style layer, a tuple of bools (st_plan_w2_diagonal)."""
        n = len(self.style_layers)
        fa = (ctypes.c_int * max(n, 1))()
        _check(self.lib.st_plan_w2_diagonal(self.handle, fa))
        return tuple(bool(v) for v in fa[:n])

    def set_w2_marginal(self, flags=None):
        """Match a 'w2' style layer on its exact per-channel marginals (st_plan_set_w2_marginal): None or False (no layer),
        True (every layer of the list - all must be 'w2') or a sequence with one bool per style layer.  A flagged layer's
        term is the mean over channels and ranks of ``(sort(f) - T)^2`` with ``T`` the style's quantile functions
        (``set_style_quantiles``): a segmented sort of the tap and one residual pass, no C x C work.  Any set flag runs the
        general closure; drops every target.  Refused together with a diagonal flag or a custom eps on the same layer, and
        while a style mask or regions are set.  Either kinds setter and ``set_taps`` clear the flags: kinds, eps, diagonal,
        then this, then the weights and targets."""
        n = len(self.style_layers)
        if flags is None or isinstance(flags, (bool, int)):
            flags = [bool(flags)] * n
        flags = list(flags)
        if len(flags) != n:
            raise ValueError(f'{len(flags)} marginal flags for {n} style layers: one per layer')
        for v in flags:
            if v not in (0, 1, False, True):
                raise ValueError(f'marginal flag {v!r}: must be a bool')
        fa = (ctypes.c_int * max(n, 1))(*[int(v) for v in flags])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_w2_marginal(self.handle, fa))

    @property
    def w2_marginal(self):
        """The marginal flag of each style layer, a tuple of bools (st_plan_w2_marginal)."""
        n = len(self.style_layers)
        fa = (ctypes.c_int * max(n, 1))()
        _check(self.lib.st_plan_w2_marginal(self.handle, fa))
        return tuple(bool(v) for v in fa[:n])

    def set_style_nearest(self, flags=None):
        """Match a 'w2' style layer on nearest style vectors (st_plan_set_style_nearest): None or False (no layer), True (every
        layer of the list - all must be 'w2') or a sequence with one bool per style layer.  A flagged layer's term is the mean
        over channels and pixels of ``|f_i - s_k*(i)|^2`` with ``s_k*(i)`` the closest of the style's feature vectors
        (``set_style_vectors``): one fused search - ``2 C N M`` flop, no N x M matrix - and one finish pass, no C x C work.  Any
        set flag runs the general closure; drops every target.  Refused together with a diagonal or marginal flag or a custom
        eps on the same layer, and while a style mask or regions are set.  Either kinds setter and ``set_taps`` clear the
        flags: kinds, eps, diagonal, marginal, then this, then the weights and targets."""
        n = len(self.style_layers)
        if flags is None or isinstance(flags, (bool, int)):
            flags = [bool(flags)] * n
        flags = list(flags)
        if len(flags) != n:
            raise ValueError(f'{len(flags)} nearest flags for {n} style layers: one per layer')
        for v in flags:
            if v not in (0, 1, False, True):
                raise ValueError(f'nearest flag {v!r}: must be a bool')
        fa = (ctypes.c_int * max(n, 1))(*[int(v) for v in flags])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_nearest(self.handle, fa))

    @property
    def style_nearest(self):
        """The nearest flag of each style layer, a tuple of bools (st_plan_style_nearest)."""
        n = len(self.style_layers)
        fa = (ctypes.c_int * max(n, 1))()
        _check(self.lib.st_plan_style_nearest(self.handle, fa))
        return tuple(bool(v) for v in fa[:n])

    def set_nearest_metric(self, names=None):
        """What the layers flagged by ``set_style_nearest`` are matched on (st_plan_set_nearest_metric): None (every layer
        'l2'), one name of ``NEAREST_METRICS`` for every flagged layer, or a sequence with one name per style layer.  'cosine':
        ``k*(i) = argmax_k <f_i, s^_k>`` on the style's unit vectors and the term ``mean_i (1 - cos(f_i, s_k*))``;
        'centered_cosine': the same after subtracting the style set's mean feature from both.  Call it after
        ``set_style_nearest`` (which resets every layer to 'l2') and before the weights and targets; drops every target.  A
        name other than 'l2' on a layer that is not flagged is refused."""
        n = len(self.style_layers)
        if names is None:
            names = [NEAREST_METRICS[0]] * n
        elif isinstance(names, str):
            flagged = self.style_nearest
            names = [names if flagged[j] else NEAREST_METRICS[0] for j in range(n)]
        names = list(names)
        if len(names) != n:
            raise ValueError(f'{len(names)} nearest metrics for {n} style layers: one per layer')
        for v in names:
            if v not in NEAREST_METRICS:
                raise ValueError(f'nearest metric {v!r}: one of {NEAREST_METRICS}')
        ma = (ctypes.c_int * max(n, 1))(*[NEAREST_METRICS.index(v) for v in names])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_nearest_metric(self.handle, ma))

    @property
    def nearest_metric(self):
        """The metric of each style layer, a tuple of names of ``NEAREST_METRICS`` (st_plan_nearest_metric)."""
        n = len(self.style_layers)
        ma = (ctypes.c_int * max(n, 1))()
        _check(self.lib.st_plan_nearest_metric(self.handle, ma))
        return tuple(NEAREST_METRICS[v] for v in ma[:n])

    def set_style_sliced(self, flags=None):
        """Match a 'w2' style layer on sliced projections (st_plan_set_style_sliced): None or False (no layer), True (every
        layer of the list - all must be 'w2') or a sequence with one bool per style layer.  A flagged layer's term is the mean
        over P random unit directions and ranks of ``(sort(R f) - T)^2`` with ``T`` the blended quantile functions of the
        style's projected feature vectors (``set_style_sliced_vectors``), new directions at every closure: the sliced
        Wasserstein loss.  Any set flag runs the general closure; drops every target and returns the options
        (``set_sliced_options``) to their defaults.  Refused together with a diagonal, marginal or nearest flag or a custom
        eps on the same layer, and while a style mask or regions are set.  Either kinds setter and ``set_taps`` clear the
        flags: kinds, eps, diagonal, marginal, nearest, then this, its options and seed, then the weights and targets."""
        n = len(self.style_layers)
        if flags is None or isinstance(flags, (bool, int)):
            flags = [bool(flags)] * n
        flags = list(flags)
        if len(flags) != n:
            raise ValueError(f'{len(flags)} sliced flags for {n} style layers: one per layer')
        for v in flags:
            if v not in (0, 1, False, True):
                raise ValueError(f'sliced flag {v!r}: must be a bool')
        fa = (ctypes.c_int * max(n, 1))(*[int(v) for v in flags])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_sliced(self.handle, fa))

    @property
    def style_sliced(self):
        """The sliced flag of each style layer, a tuple of bools (st_plan_style_sliced)."""
        n = len(self.style_layers)
        fa = (ctypes.c_int * max(n, 1))()
        _check(self.lib.st_plan_style_sliced(self.handle, fa))
        return tuple(bool(v) for v in fa[:n])

    def set_sliced_options(self, index, projections=None, resample=True):
        """Flagged style entry ``index``: the number of directions (None or 0: the tap's channels; else a multiple of 64 in
        [64, 512]) and whether every closure draws new ones (st_plan_set_sliced_options).  Drops that entry's target."""
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_sliced_options(self.handle, int(index), int(projections or 0), int(bool(resample))))

    def set_sliced_seed(self, seed):
        """The seed of the flagged entries' directions; the epoch returns to 0 and their targets are dropped
        (st_plan_set_sliced_seed): set it before the style vectors."""
        _check(self.lib.st_plan_set_sliced_seed(self.handle, int(seed) & 0xffffffffffffffff))

    def _layer_values(self, entry, ctype):
        ca, sa = (ctype * max(len(self.content_layers), 1))(), (ctype * max(len(self.style_layers), 1))()
        _check(entry(self.handle, ca, sa))
        return tuple(ca[:len(self.content_layers)]), tuple(sa[:len(self.style_layers)])

    def _read_loss_kinds(self):
        c, s = ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_loss_kinds(self.handle, ctypes.byref(c), ctypes.byref(s)))
        self.content_loss = CONTENT_LOSSES[c.value] if c.value >= 0 else self.content_losses
        self.style_loss = STYLE_LOSSES[s.value] if s.value >= 0 else self.style_losses

    @property
    def content_losses(self):
        """The loss kind of each content layer, a tuple of names (st_plan_layer_loss_kinds)."""
        return tuple(CONTENT_LOSSES[k] for k in self._layer_values(self.lib.st_plan_layer_loss_kinds, ctypes.c_int)[0])

    @property
    def style_losses(self):
        """The loss kind of each style layer."""
        return tuple(STYLE_LOSSES[k] for k in self._layer_values(self.lib.st_plan_layer_loss_kinds, ctypes.c_int)[1])

    @property
    def content_eps(self):
        """The effective eps of each content layer's module (st_plan_loss_eps), None for an 'mse' layer."""
        return tuple(None if v < 0 else v for v in self._layer_values(self.lib.st_plan_loss_eps, ctypes.c_float)[0])

    @property
    def style_eps(self):
        """The effective eps of each style layer's module."""
        return self._layer_values(self.lib.st_plan_loss_eps, ctypes.c_float)[1]

    def term_losses(self):
        """The weighted terms of the last closure in SumLoss order - content layers, style layers, tv - as a device tensor
        (st_plan_term_losses; a copy)."""
        data, n = ctypes.c_void_p(), ctypes.c_int()
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_term_losses(self.handle, ctypes.byref(data), ctypes.byref(n)))
            out = torch.empty(n.value, device=self.device, dtype=torch.float32)
            _copy_d2d(out, data.value)
        return out

    def device_bytes(self):
        return int(self.lib.st_plan_device_bytes(self.handle))

    def debug_read(self, what, count):
        """Diagnostic: `count` floats of an internal buffer, as a CPU tensor (st_plan_debug_read in include/st_amd.h).
        0: the TV kernels' per-workgroup partial sums.  2 (`count` must be 64): the fp16x3 operand bounds of the last
        pass, one float per bound word - words 0 .. 12 max |y| of the 13 ReLU outputs, 16 .. 28 max |g| of their
        (ReLU-masked) gradients, 32 .. 35 max |g| of the 4 pooled maps' gradients, 48 .. 63 the style heads'; a pooled map
        shares the word of the convolution that feeds its pool, that convolution's gradient shares the pool's g word.  Read
        them after ``forward``, ``backward`` or ``loss_and_grad``: a ``step`` clears them in its tail.  16 + i: the
        gradient map of the i-th of the 17 taps in network order (`count`: its C * h * w)."""
        import numpy as np
        if int(what) == 2 and int(count) != 64:
            raise ValueError(f'debug_read(2, {count}): the plan has 64 operand bounds')
        buf = np.empty(int(count), dtype=np.float32)
        _check(self.lib.st_plan_debug_read(self.handle, int(what), buf.ctypes.data_as(ctypes.POINTER(ctypes.c_float)), int(count)))
        return torch.from_numpy(buf)

    def _img(self, image):
        assert image.shape[-3:] == (3, self.height, self.width), (image.shape, self.height, self.width)
        return _ptr(image)

    def forward(self, image, last_layer=29):
        self.forward_count += 1
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_forward(self.handle, self._img(image), int(last_layer), _stream()))

    def backward(self, layers, grads, grad_out=None):
        """The vector-Jacobian product of the last ``forward`` (st_plan_backward): ``grads[i]`` is the gradient with respect
        to the tap ``layers[i]`` (any ReLU or pool index up to that forward's ``last_layer``, each once; a contiguous fp32
        tensor of the tap's shape on this device).  Returns the image gradient [1, 3, H, W] - written into ``grad_out`` when
        given, not added to it.  Raises HipLibraryError when a closure (loss_and_grad, step, ...) has run on this plan since
        the forward: run ``forward`` again."""
        layers, grads = [int(layer) for layer in layers], list(grads)
        assert len(layers) == len(grads), (len(layers), len(grads))
        if grad_out is None:
            grad_out = torch.empty((1, 3, self.height, self.width), device=self.device, dtype=torch.float32)
        assert grad_out.numel() == 3 * self.height * self.width
        for layer, g in zip(layers, grads):          # the library reads C * h * w floats behind each pointer
            data, c, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
            _check(self.lib.st_plan_feature(self.handle, layer, ctypes.byref(data), ctypes.byref(c), ctypes.byref(h),
                                            ctypes.byref(w)))
            assert g.numel() == c.value * h.value * w.value, (layer, tuple(g.shape), (c.value, h.value, w.value))
        for t in (*grads, grad_out):                 # (_ptr checks fp32 and contiguous; the pointers are read on this device)
            assert t.is_cuda and self.device.index in (None, t.device.index), (t.device, self.device)
        la = (ctypes.c_int * max(len(layers), 1))(*layers)
        ga = (ctypes.c_void_p * max(len(grads), 1))(*[_ptr(g).value for g in grads])
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_backward(self.handle, len(layers), la, ga, _ptr(grad_out), _stream()))
        return grad_out

    def feature(self, layer):
        """Copy of a tap as a [1, C, h, w] tensor."""
        data, c, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_feature(self.handle, int(layer), ctypes.byref(data), ctypes.byref(c),
                                        ctypes.byref(h), ctypes.byref(w)))
        out = torch.empty((1, c.value, h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)   # D2D on the current stream from the ABI's borrowed pointer
        return out

    def moments(self, layer):
        """(mean [C], srm [C, C]) of a tap of the last forward (st_plan_moments): any of ``TAPS``."""
        if int(layer) not in TAPS:
            raise ValueError(f'features[{int(layer)}] is not one of the taps {TAPS}')
        c = 64 if layer < 5 else 128 if layer < 10 else 256 if layer < 19 else 512
        mean = torch.empty(c, device=self.device, dtype=torch.float32)
        srm = torch.empty((c, c), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_moments(self.handle, int(layer), _ptr(mean), _ptr(srm), _stream()))
        return mean, srm

    def tap_pixels(self, layer):
        """h w of a tap at this plan's size."""
        data, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_feature(self.handle, int(layer), ctypes.byref(data), None, ctypes.byref(h), ctypes.byref(w)))
        return h.value * w.value

    def quantiles(self, layer):
        """The sorted tap of the last forward, [C, N] with N = h w: every channel's values in ascending order, its quantile
        function (st_op_channel_sort on the tap) - what ``set_style_quantiles`` takes, beside ``moments``."""
        if int(layer) not in TAPS:
            raise ValueError(f'features[{int(layer)}] is not one of the taps {TAPS}')
        return op_channel_sort(self.feature(layer)[0])[0]

    def set_style_quantiles(self, index, q):
        """The target of a style layer flagged by ``set_w2_marginal``: ``q`` [C, n_q], sorted rows - a style tap's
        ``quantiles``, or a weighted blend of several - resampled to this plan's pixel count (st_plan_set_style_quantiles)."""
        q = q.to(device=self.device, dtype=torch.float32).contiguous()
        if q.ndim != 2:
            raise ValueError(f'quantiles of shape {tuple(q.shape)}: [C, n_q]')
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_quantiles(self.handle, int(index), _ptr(q), int(q.shape[1]), _stream()))

    def style_quantiles(self, index):
        """Copy of a flagged layer's resampled target, [C, N] (st_plan_style_quantiles)."""
        data, c, n = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_longlong()
        _check(self.lib.st_plan_style_quantiles(self.handle, int(index), ctypes.byref(data), ctypes.byref(c), ctypes.byref(n)))
        out = torch.empty((c.value, n.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out

    def set_style_vectors(self, index, vectors):
        """The target of a style layer flagged by ``set_style_nearest``: ``vectors`` [C, M] (or [C, h, w]), the style's feature
        vectors as columns - a style tap (``feature(layer)[0]``), or several concatenated along the columns
        (st_plan_set_style_vectors).  M need not be this plan's pixel count."""
        vectors = vectors.to(device=self.device, dtype=torch.float32)
        if vectors.ndim == 3:
            vectors = vectors.flatten(1)
        if vectors.ndim != 2:
            raise ValueError(f'style vectors of shape {tuple(vectors.shape)}: [C, M]')
        vectors = vectors.contiguous()
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_vectors(self.handle, int(index), _ptr(vectors), int(vectors.shape[1]), _stream()))

    def nearest_indices(self, layer):
        """Copy of the last closure's matches of the flagged style layer ``layer`` (a features index of ``style_layers``), [N]
        int64: the style vector each pixel of the tap was matched to (st_plan_nearest_indices)."""
        if int(layer) not in self.style_layers:
            raise ValueError(f'features[{int(layer)}] is not one of the style layers {tuple(self.style_layers)}')
        index = list(self.style_layers).index(int(layer))
        data, n = ctypes.c_void_p(), ctypes.c_longlong()
        _check(self.lib.st_plan_nearest_indices(self.handle, index, ctypes.byref(data), ctypes.byref(n)))
        out = torch.empty((n.value,), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out.to(torch.int64)

    def set_style_sliced_vectors(self, index, vectors, weights=None):
        """The target of a style layer flagged by ``set_style_sliced``: ``vectors`` is one [C, M] (or [C, h, w]) tensor or a
        sequence of them, one per style image - each a style tap (``feature(layer)[0]``) - and ``weights`` one non-negative
        number per image (None: equal).  The plan keeps the vectors and derives the target from them under the directions of
        every epoch (st_plan_set_style_sliced_vectors).  M need not be this plan's pixel count."""
        if torch.is_tensor(vectors):
            vectors = [vectors]
        kept = []
        for v in vectors:
            v = v.to(device=self.device, dtype=torch.float32)
            if v.ndim == 3:
                v = v.flatten(1)
            if v.ndim != 2:
                raise ValueError(f'style vectors of shape {tuple(v.shape)}: [C, M]')
            kept.append(v.contiguous())
        n = len(kept)
        if weights is not None and len(weights) != n:
            raise ValueError(f'{len(weights)} weights for {n} style images: one per image')
        pa = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in kept])
        ma = (ctypes.c_longlong * max(n, 1))(*[int(v.shape[1]) for v in kept])
        wa = (ctypes.c_float * max(n, 1))(*[float(w) for w in weights]) if weights is not None else None
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_sliced_vectors(self.handle, int(index), n, pa, ma, wa, _stream()))

    def _sliced_index(self, layer):
        if int(layer) not in self.style_layers:
            raise ValueError(f'features[{int(layer)}] is not one of the style layers {tuple(self.style_layers)}')
        return list(self.style_layers).index(int(layer))

    def sliced_directions(self, layer):
        """(copy of the directions R [P, C] the last closure used for the flagged style layer ``layer`` - a features index of
        ``style_layers``; before any closure those the setter drew - and their epoch) - st_plan_sliced_directions."""
        data, proj, c, epoch = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_ulonglong()
        _check(self.lib.st_plan_sliced_directions(self.handle, self._sliced_index(layer), ctypes.byref(data), ctypes.byref(proj),
                                                  ctypes.byref(c), ctypes.byref(epoch)))
        out = torch.empty((proj.value, c.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out, int(epoch.value)

    def sliced_target(self, layer):
        """Copy of the flagged style layer's target under those directions, [P, N] (st_plan_sliced_target)."""
        data, proj, n = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_longlong()
        _check(self.lib.st_plan_sliced_target(self.handle, self._sliced_index(layer), ctypes.byref(data), ctypes.byref(proj), ctypes.byref(n)))
        out = torch.empty((proj.value, n.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out

    def set_style_mask(self, mask):
        """A spatial mask for the style statistics (st_plan_set_style_mask): a [height, width] tensor with values in [0, 1]
        at the plan's image size, or None to clear it.  While it is set every style head of every closure and step, and
        ``moments``, take the mask-weighted moments of their tap (the mask averaged down 2 x 2 to the tap's resolution).
        Raises HipLibraryError on a strip plan, for a NaN or a value outside [0, 1], and when a level of the pyramid sums
        to 0; a refused mask leaves the plan without one."""
        with torch.cuda.device(self.device):
            if mask is None:
                _check(self.lib.st_plan_set_style_mask(self.handle, None, _stream()))
                return
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != (self.height, self.width):
                raise ValueError(f'style mask of shape {tuple(mask.shape)}: the plan is {self.height} x {self.width}')
            mask = mask.to(self.device, torch.float32).contiguous()
            _check(self.lib.st_plan_set_style_mask(self.handle, _ptr(mask), _stream()))

    def style_mask_level(self, level):
        """(sqrt of level ``level`` of the style mask as an [h, w] tensor - a copy -, the level's sum) as the plan keeps them
        (st_plan_style_mask): level k serves the taps behind k pools.  Raises HipLibraryError when no mask is set."""
        data, h, w, total = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        _check(self.lib.st_plan_style_mask(self.handle, int(level), ctypes.byref(data), ctypes.byref(h), ctypes.byref(w),
                                           ctypes.byref(total)))
        out = torch.empty((h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out, total.value

    def set_style_regions(self, masks):
        """Several style regions with a style each (st_plan_set_style_regions): a list of 1 to 4 [height, width] tensors with
        values in [0, 1] at the plan's image size, or None (or an empty list) to clear them.  Region r's targets are set with
        ``set_region_style_target``, its weight with ``set_region_weights`` (1 / R each after every call here); each style
        term is then the sum over the regions of the layer's module on the region's mask-weighted moments against the
        region's target.  Raises ValueError for a mask of another size, HipLibraryError on a strip plan, for more than 4
        regions, while a style mask is set, for a NaN or a value outside [0, 1] and when a level of a region's pyramid sums
        to 0; a refused call leaves the plan without regions."""
        with torch.cuda.device(self.device):
            if masks is None or len(masks) == 0:
                _check(self.lib.st_plan_set_style_regions(self.handle, 0, None, _stream()))
                return
            held = []
            for r, mask in enumerate(masks):
                mask = torch.as_tensor(mask)
                if tuple(mask.shape) != (self.height, self.width):
                    raise ValueError(f'style region {r}: mask of shape {tuple(mask.shape)}: the plan is {self.height} x {self.width}')
                held.append(mask.to(self.device, torch.float32).contiguous())
            ptrs = (ctypes.c_void_p * len(held))(*[_ptr(m).value for m in held])
            _check(self.lib.st_plan_set_style_regions(self.handle, len(held), ptrs, _stream()))

    def style_region_level(self, region, level):
        """(sqrt of level ``level`` of region ``region``'s mask as an [h, w] tensor - a copy -, the level's sum) as the plan
        keeps them (st_plan_style_region).  Raises HipLibraryError when no regions are set."""
        data, h, w, total = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_double()
        _check(self.lib.st_plan_style_region(self.handle, int(region), int(level), ctypes.byref(data), ctypes.byref(h),
                                             ctypes.byref(w), ctypes.byref(total)))
        out = torch.empty((h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out, total.value

    def set_region_style_target(self, region, index, mean, srm):
        """``set_style_target`` for region ``region`` of the regions in force (st_plan_set_region_style_target)."""
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_region_style_target(self.handle, int(region), int(index), _ptr(mean.contiguous()),
                                                            _ptr(srm.contiguous()), _stream()))

    def set_region_weights(self, weights):
        """The regions' weights, one per region in force, used as given; None restores 1 / R each (st_plan_set_region_weights)."""
        if weights is None:
            _check(self.lib.st_plan_set_region_weights(self.handle, None))
            return
        ws = [float(w) for w in weights]
        count = ctypes.c_int()
        _check(self.lib.st_plan_region_terms(self.handle, ctypes.byref(ctypes.c_void_p()), ctypes.byref(count), None))
        if len(ws) != count.value:
            raise ValueError(f'{len(ws)} region weights for {count.value} style regions')
        _check(self.lib.st_plan_set_region_weights(self.handle, (ctypes.c_float * len(ws))(*ws)))

    def region_term_losses(self):
        """The weighted term of every (region, style layer) of the last closure as an [R, n_style] device tensor
        (st_plan_region_terms; a copy): column j sums, over the regions in order, to style term j of ``term_losses``."""
        data, regions, styles = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_region_terms(self.handle, ctypes.byref(data), ctypes.byref(regions), ctypes.byref(styles)))
            out = torch.empty((regions.value, styles.value), device=self.device, dtype=torch.float32)
            if out.numel():
                _copy_d2d(out, data.value)
        return out

    def _set_weight_map(self, entry, what, mask):
        with torch.cuda.device(self.device):
            if mask is None:
                _check(entry(self.handle, None, _stream()))
                return
            mask = torch.as_tensor(mask)
            if tuple(mask.shape) != (self.height, self.width):
                raise ValueError(f'{what} of shape {tuple(mask.shape)}: the plan is {self.height} x {self.width}')
            mask = mask.to(self.device, torch.float32).contiguous()
            _check(entry(self.handle, _ptr(mask), _stream()))

    def set_content_mask(self, mask):
        """A spatial weight map for the content terms (st_plan_set_content_mask): a [height, width] tensor with values in
        [0, 1] at the plan's image size, or None to clear it.  While it is set every content term of every closure and step
        weighs (F - T) per pixel with the map averaged down 2 x 2 to its tap's resolution; the normaliser stays the element
        count.  Every target stays.  Raises ValueError for another size, HipLibraryError on a strip plan, for a NaN or a
        value outside [0, 1] and for an all-zero map; a refused map leaves the plan without one."""
        self._set_weight_map(self.lib.st_plan_set_content_mask, 'content map', mask)

    def content_mask_level(self, level):
        """Level ``level`` of the content map as the plan keeps it, an [h, w] tensor (a copy; st_plan_content_mask): level k
        serves the content layers behind k pools.  Raises HipLibraryError when no content map is set."""
        data, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_content_mask(self.handle, int(level), ctypes.byref(data), ctypes.byref(h), ctypes.byref(w)))
        out = torch.empty((h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out

    def set_tv_mask(self, mask):
        """A spatial weight map for the TV term (st_plan_set_tv_mask): a [height, width] tensor with values in [0, 1] at the
        plan's image size, or None to clear it.  While it is set each squared difference of the TV term is weighed by the
        mean of the map at its two end points.  Raises as ``set_content_mask`` does."""
        self._set_weight_map(self.lib.st_plan_set_tv_mask, 'TV map', mask)

    def tv_mask(self):
        """The TV map in force as an [height, width] tensor (a copy, equal to what was set bit for bit; st_plan_tv_mask).
        Raises HipLibraryError when no TV map is set."""
        data, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_tv_mask(self.handle, ctypes.byref(data), ctypes.byref(h), ctypes.byref(w)))
        out = torch.empty((h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out

    def set_laplacian(self, content_image, pools=(4,), weight=1.0):
        """A Laplacian loss on average-pooled images (st_plan_set_laplacian): ``content_image`` a [3, height, width] (or
        [1, 3, height, width]) tensor at the plan's size, or None to clear the term; ``pools`` 1 to 4 distinct pool sizes, each
        leaving a pooled map of at least 2 x 2; ``weight`` finite and > 0.  While it is set every closure and step adds
        ``weight * mean((L(avg_pool(x, p)) - L(avg_pool(content, p))) ** 2)`` per pool size onto the image-space slot (the TV
        term's) and its gradient onto the image gradient.  Every target stays.  Raises ValueError for another size,
        HipLibraryError for what the library refuses (a strip plan, the pools, the weight); a refused call leaves the plan
        without a Laplacian."""
        with torch.cuda.device(self.device):
            if content_image is None:
                _check(self.lib.st_plan_set_laplacian(self.handle, None, 0, None, 0.0, _stream()))
                return
            content_image = torch.as_tensor(content_image)
            if tuple(content_image.shape[-3:]) != (3, self.height, self.width) or content_image.numel() != 3 * self.height * self.width:
                raise ValueError(f'content image of shape {tuple(content_image.shape)}: the plan is 3 x {self.height} x {self.width}')
            content_image = content_image.to(self.device, torch.float32).contiguous()
            pools = [int(p) for p in pools]
            pa = (ctypes.c_int * max(len(pools), 1))(*pools)
            _check(self.lib.st_plan_set_laplacian(self.handle, _ptr(content_image), len(pools), pa, float(weight), _stream()))

    def laplacian_target(self, k):
        """The target ``L(avg_pool(content, p_k))`` of the k-th pool size as a [3, h, w] tensor (a copy; st_plan_laplacian).
        Raises HipLibraryError when no Laplacian is set."""
        data, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_laplacian(self.handle, int(k), ctypes.byref(data), ctypes.byref(h), ctypes.byref(w)))
        out = torch.empty((3, h.value, w.value), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _copy_d2d(out, data.value)
        return out

    def laplacian_terms(self):
        """``[tv alone, term_p0, term_p1, ...]`` of the last closure as a device tensor (a copy; st_plan_laplacian_terms): the
        last entry of ``term_losses`` is their fp32 sum in this order.  Raises HipLibraryError when no Laplacian is set."""
        data, n = ctypes.c_void_p(), ctypes.c_int()
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_laplacian_terms(self.handle, ctypes.byref(data), ctypes.byref(n)))
            out = torch.empty(n.value, device=self.device, dtype=torch.float32)
            _copy_d2d(out, data.value)
        return out

    def set_content_target(self, feat, index=0):
        """The target of content layer ``index`` of the configured list (st_plan_set_content_target_at)."""
        data, c, h, w = ctypes.c_void_p(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(self.lib.st_plan_feature(self.handle, self.content_layers[int(index)], ctypes.byref(data), ctypes.byref(c),
                                        ctypes.byref(h), ctypes.byref(w)))
        assert feat.numel() == c.value * h.value * w.value, (tuple(feat.shape), (c.value, h.value, w.value))
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_content_target_at(self.handle, int(index), _ptr(feat.contiguous()), _stream()))

    def set_content_target_from_forward(self):
        """Every configured content layer's target from the maps of the current forward."""
        for index, layer in enumerate(self.content_layers):
            data = ctypes.c_void_p()
            _check(self.lib.st_plan_feature(self.handle, layer, ctypes.byref(data), None, None, None))
            with torch.cuda.device(self.device):
                _check(self.lib.st_plan_set_content_target_at(self.handle, index, data, _stream()))

    def set_style_target(self, index, mean, srm):
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_set_style_target(self.handle, int(index), _ptr(mean.contiguous()),
                                                     _ptr(srm.contiguous()), _stream()))

    def set_loss_weights(self, content_weight, style_layer_weights, tv_weight):
        """``content_weight``: one float for every content layer, or one per layer; ``style_layer_weights``: one per style
        layer (st_plan_set_tap_weights)."""
        nc, ns = len(self.content_layers), len(self.style_layers)
        try:                                        # any sequence (list, tuple, numpy array, tensor), or one number
            cws = [float(w) for w in content_weight]
        except TypeError:
            cws = [float(content_weight)] * nc
        sws = [float(w) for w in style_layer_weights]
        # One entry serves every configuration.  The lists are still compared, for one reason: with the default layers fewer
        # than 5 style weights have always meant "the rest are zero", while for any other lists a count mismatch is an error.
        if (tuple(self.content_layers), tuple(self.style_layers)) == (DEFAULT_CONTENT_LAYERS, DEFAULT_STYLE_LAYERS):
            sws += [0.0] * (ns - len(sws))
        if len(cws) != nc or len(sws) != ns:
            raise ValueError(f'{len(cws)} content and {len(sws)} style weights for {nc} content and {ns} style layers')
        ca, sa = (ctypes.c_float * max(nc, 1))(*cws), (ctypes.c_float * max(ns, 1))(*sws)
        _check(self.lib.st_plan_set_tap_weights(self.handle, ca, sa, float(tv_weight)))

    def loss_and_grad(self, image, grad_out=None):
        """Returns (losses[8] device tensor: 7 weighted terms + total, grad [like image])."""
        if grad_out is None:
            grad_out = torch.empty_like(image)
        self.forward_count += 1
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_loss_and_grad(self.handle, self._img(image), _ptr(grad_out),
                                                  _ptr(self.losses), _stream()))
        return self.losses, grad_out

    def step(self, image, exp_avg, exp_avg_sq, ema_value, step, lr, beta1=0.9, beta2=0.99, eps=1e-8,
             ema_decay=0.99):
        self.forward_count += 1
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_step(self.handle, self._img(image), _ptr(exp_avg), _ptr(exp_avg_sq),
                                         _ptr(ema_value), int(step), float(lr), float(beta1), float(beta2),
                                         float(eps), float(ema_decay), _ptr(self.losses), _stream()))
        return self.losses

    def apply_update(self, image, grad, exp_avg, exp_avg_sq, ema_value, step, lr, beta1=0.9, beta2=0.99, eps=1e-8,
                     ema_decay=0.99):
        """Only the update of ``step`` - Adam + clamp + EMA - on an externally supplied gradient (st_plan_apply_update)."""
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_apply_update(self.handle, self._img(image), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq),
                                                 _ptr(ema_value), int(step), float(lr), float(beta1), float(beta2),
                                                 float(eps), float(ema_decay), _stream()))

    def range_guard(self, image):
        """Activation-aware dynamic-range check of the fp16x3 convolutions on ``image`` (st_plan_range_guard): returns the
        ([13], [13]) forward / data-gradient layers this call moved to bf16x6 (cold path, synchronous)."""
        fwd, bwd = (ctypes.c_int * 13)(), (ctypes.c_int * 13)()
        self.forward_count += 1
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_range_guard(self.handle, self._img(image), fwd, bwd, _stream()))
        return list(fwd), list(bwd)

    def set_graph(self, on=True):
        _check(self.lib.st_plan_set_graph(self.handle, 1 if on else 0))

    def profile_enable(self, on=True):
        _check(self.lib.st_plan_profile_enable(self.handle, 1 if on else 0))

    HBM_KERNELS = ('conv1_1 forward (+ normalize)', 'conv1_1 data gradient (+ pad fold)', 'max-pool backward (4 levels)',
                   'Adam + clamp + EMA', 'TV loss + gradient', 'relu1_1 Gram + mean', 'content MSE + gradient',
                   "style heads' 1x1 gradient step (5 taps)")

    def profile_read_hbm(self):
        """{kernel: (launches, ms, algorithmic bytes)} of the HBM-bound kernels since the last profile_read()
        (call BEFORE profile_read, which recycles the events)."""
        out = {}
        for cat, name in enumerate(self.HBM_KERNELS):
            n, ms, by = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
            _check(self.lib.st_plan_profile_read_hbm(self.handle, cat, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(by)))
            out[name] = (n.value, ms.value, by.value)
        return out

    def profile_read(self):
        n, ms, fl = ctypes.c_longlong(), ctypes.c_double(), ctypes.c_double()
        _check(self.lib.st_plan_profile_read(self.handle, ctypes.byref(n), ctypes.byref(ms), ctypes.byref(fl)))
        return n.value, ms.value, fl.value


class LBFGS:
    """State of the native ``optimizer='lbfgs'`` step (st_lbfgs_* in include/st_amd.h):
    ``torch.optim.LBFGS(max_iter=1, history_size=10)`` for ONE parameter tensor, every decision of ``LBFGS.step`` taken on
    the device.  The state - ring of curvature pairs, Gram matrix, partial sums, counters - is one torch tensor, so
    ``torch.cuda.max_memory_allocated`` counts it.

    ``like`` may be ONE RANK'S STRIP of the parameter (``rank`` of ``world``): ``update_strip`` / ``step_strip`` then complete
    the inner products over the ranks with one all-gather of 72 doubles per rank (st_qn_strip_* in include/st_amd.h).  The
    state is the unsharded layout with ``world`` such records behind it, so every method works on it."""

    EXITS = ('moved', 'gradient', 'change')      # exit_code of info(): the step moved / tolerance_grad / tolerance_change

    def __init__(self, like, rank=0, world=1):
        self.lib = load_library()
        self.device = like.device
        self.count = like.numel()
        self.rank, self.world = int(rank), int(world)
        nbytes = int(self.lib.st_qn_strip_state_bytes(self.count, self.world))
        if nbytes <= 0 or not 0 <= self.rank < self.world:
            raise ValueError(f'LBFGS: rank {rank} of {world} ranks (1 ... 8) for {self.count} elements')
        self._exchange = Exchange()
        self.state = torch.empty((nbytes + 3) // 4, device=self.device, dtype=torch.float32)
        self.reset()

    def _state(self):
        return ctypes.c_void_p(self.state.data_ptr())

    def reset(self):
        """A fresh optimiser (the reference makes a new LBFGS per scale)."""
        with torch.cuda.device(self.device):
            _check(self.lib.st_lbfgs_reset(self._state(), self.count, _stream()))

    def step(self, plan, image, ema_value, ema_decay):
        """closure + LBFGS.step + EMA.update(image) (st_plan_lbfgs_step); returns the plan's 8 losses (device)."""
        assert image.numel() == self.count
        plan.forward_count += 1
        with torch.cuda.device(self.device):
            _check(self.lib.st_plan_lbfgs_step(plan.handle, plan._img(image), self._state(), _ptr(ema_value),
                                               float(ema_decay), _ptr(plan.losses), _stream()))
        return plan.losses

    def update(self, image, grad, ema_value=None, ema_decay=0.99):
        """LBFGS.step on an externally supplied gradient (+ EMA.update when ``ema_value`` is given): st_lbfgs_update."""
        assert image.numel() == self.count and grad.numel() == self.count
        with torch.cuda.device(self.device):
            _check(self.lib.st_lbfgs_update(self._state(), self.count, _ptr(image), _ptr(grad), _ptr(ema_value),
                                            float(ema_decay), _stream()))

    def strip_dots(self, grad):
        """First launch of a strip's step (st_qn_strip_dots): this rank's record lands in its slot of the state's gather
        area; returns the kind-6 exchange descriptor that must be performed before ``strip_apply``."""
        assert grad.numel() == self.count
        with torch.cuda.device(self.device):
            _check(self.lib.st_qn_strip_dots(self._state(), self.count, self.rank, self.world, _ptr(grad),
                                             ctypes.byref(self._exchange), _stream()))
        return self._exchange

    def strip_apply(self, image, grad, ema_value=None, ema_decay=0.99):
        """Second and third launch (st_qn_strip_apply): the records added in rank order, LBFGS.step's scalar work, the move
        and EMA.update."""
        assert image.numel() == self.count and grad.numel() == self.count
        with torch.cuda.device(self.device):
            _check(self.lib.st_qn_strip_apply(self._state(), self.count, self.world, _ptr(image), _ptr(grad),
                                              _ptr(ema_value), float(ema_decay), _stream()))

    def update_strip(self, image, grad, fabric, ema_value=None, ema_decay=0.99):
        """LBFGS.step on this rank's strip of an externally supplied gradient, the descriptor form: dots, the all-gather
        through ``fabric.apply`` (a sharding.DistFabric), apply."""
        ex = self.strip_dots(grad)
        fabric.apply(ex, self.device)
        self.strip_apply(image, grad, ema_value, ema_decay)

    def step_strip(self, plan, fabric, image, grad, ema_value, ema_decay):
        """closure + LBFGS.step + EMA.update on this rank's strip (``plan``: a sharding.StripPlan; ``grad``: the buffer the
        closure writes).  Over a sharding.NativeFabric ONE call (st_plan_qn_strip_step: the in-library transport issues
        the all-gather); otherwise closure_begin, run_phases, update_strip.  Returns the plan's 8 losses (device)."""
        from . import sharding
        assert image.numel() == self.count
        if isinstance(fabric, sharding.NativeFabric):
            plan._inflight = (image, grad)
            with torch.cuda.device(self.device):
                _check(self.lib.st_plan_qn_strip_step(plan.handle, fabric.handle, plan._img(image), _ptr(grad), self._state(),
                                                      _ptr(ema_value), float(ema_decay), _stream()))
        else:
            plan.closure_begin(image, grad)
            sharding.run_phases(plan, fabric)
            self.update_strip(image, grad, fabric, ema_value, ema_decay)
        return plan.losses

    def info(self):
        """Counters and the last step's flags (synchronises): dict(n_iter, history, exit, accepted, t, gtd)."""
        n, h, e, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        t, gtd = ctypes.c_double(), ctypes.c_double()
        with torch.cuda.device(self.device):
            _check(self.lib.st_lbfgs_info(self._state(), self.count, ctypes.byref(n), ctypes.byref(h), ctypes.byref(e),
                                          ctypes.byref(a), ctypes.byref(t), ctypes.byref(gtd), _stream()))
        return {'n_iter': n.value, 'history': h.value, 'exit': self.EXITS[e.value], 'accepted': bool(a.value),
                't': t.value, 'gtd': gtd.value}


class Head:
    """A standalone style head (st_head): StyleLossW2 (``kind='w2'``) or StyleLoss (``kind='gram'``) on a dense fp32
    [C, h, w] tensor outside any plan - what style_transfer/losses.py runs on an eligible HIP tensor.  Every tensor
    argument is a contiguous fp32 tensor on the head's device with a 16-byte aligned pointer; ``upstream`` is a 0-dim or
    one-element DEVICE tensor (autograd's grad_output) that is never read on the host."""

    KINDS = ('w2', 'gram', 'moments')       # 'moments': a head for ``moments`` alone (get_target), no forward / backward workspaces

    def __init__(self, kind, channels, height, width, device, precision='fp16x3'):
        self.lib = load_library()
        self.kind, self.precision = kind, precision
        self.shape = (int(channels), int(height), int(width))
        self.device = torch.device(device)
        h = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(self.lib.st_head_create(ctypes.byref(h), self.KINDS.index(kind), *self.shape, Net.PRECISIONS[precision]))
        self.handle = h
        self.state_floats = int(self.lib.st_head_state_floats(h))

    def __del__(self):
        h, self.handle = getattr(self, 'handle', None), None
        if h and self.lib is not None:
            self.lib.st_head_destroy(h)

    def device_bytes(self):
        return int(self.lib.st_head_device_bytes(self.handle))

    def _feat(self, feat):
        assert feat.numel() == self.shape[0] * self.shape[1] * self.shape[2], (tuple(feat.shape), self.shape)
        return _ptr(feat)

    def moments(self, feat, mean=True):
        """(mean [C] or None, srm [C, C]) of ``feat`` (st_head_moments): StyleLossW2.get_target / StyleLoss.get_target."""
        c = self.shape[0]
        mean_out = torch.empty(c, device=self.device, dtype=torch.float32) if mean else None
        srm = torch.empty((c, c), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _check(self.lib.st_head_moments(self.handle, self._feat(feat), _ptr(mean_out), _ptr(srm), _stream()))
        return mean_out, srm

    def forward(self, feat, targets, eps, need_grad=True):
        """(loss [0-dim device tensor, unweighted], state or None) - st_head_forward.  ``targets``: (mean, cov, cov_sqrt) of
        a StyleLossW2, (gram,) of a StyleLoss - the module's buffers, read in place.  ``state`` is what ``backward`` needs:
        (Ssym, b) and the operand bound, one tensor of ``state_floats`` floats owned by the caller."""
        loss = torch.empty((), device=self.device, dtype=torch.float32)
        state = torch.empty(self.state_floats, device=self.device, dtype=torch.float32) if need_grad else None
        if self.kind == 'w2':
            mean_t, cov_t, root_t = targets
            ptrs = (_ptr(mean_t), _ptr(cov_t), _ptr(root_t), None)
        else:
            ptrs = (None, None, None, _ptr(targets[0]))
        with torch.cuda.device(self.device):
            _check(self.lib.st_head_forward(self.handle, self._feat(feat), *ptrs, float(eps), _ptr(loss), _ptr(state), _stream()))
        return loss, state

    def backward(self, feat, state, upstream):
        """upstream * (Ssym F + b 1^T) as a new tensor of ``feat``'s shape (st_head_backward)."""
        grad = torch.empty(feat.shape, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _check(self.lib.st_head_backward(self.handle, self._feat(feat), _ptr(state), _ptr(upstream), _ptr(grad), _stream()))
        return grad


def _copy_d2d(dst, src_ptr):
    """Device-to-device copy from a borrowed raw pointer into a torch tensor (same device)."""
    hip = _hip_runtime()
    rc = hip.hipMemcpyAsync(ctypes.c_void_p(dst.data_ptr()), ctypes.c_void_p(src_ptr),
                            ctypes.c_size_t(dst.numel() * dst.element_size()), 3,
                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if rc != 0:
        raise HipLibraryError(f'hipMemcpyAsync failed with code {rc}')


_hiprt = None


def _hip_runtime():
    global _hiprt
    if _hiprt is None:
        for name in ('libamdhip64.so', '/opt/rocm/lib/libamdhip64.so', 'libamdhip64.so.7', 'libamdhip64.so.6'):
            try:
                _hiprt = ctypes.CDLL(name)
                break
            except OSError:
                continue
        if _hiprt is None:
            raise HipLibraryError('libamdhip64.so not found')
        _hiprt.hipMemcpyAsync.restype = ctypes.c_int
        _hiprt.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                                          ctypes.c_void_p]
    return _hiprt


# ---- standalone operators (kernel-level parity tests) ------------------------------------------
def op_sqrtm_ns(a):
    lib = load_library()
    n = a.shape[-1]
    root = torch.empty(a.shape, dtype=a.dtype, device=a.device)       # (empty_like would keep a transposed view's strides)
    with torch.cuda.device(a.device):
        _check(lib.st_op_sqrtm_ns(_ptr(a.contiguous()), _ptr(root), n, _stream()))
    return root


def op_sqrtm_ns_backward(root, grad_root):
    lib = load_library()
    n = root.shape[-1]
    ga = torch.empty(root.shape, dtype=root.dtype, device=root.device)
    with torch.cuda.device(root.device):
        _check(lib.st_op_sqrtm_ns_backward(_ptr(root.contiguous()), _ptr(grad_root.contiguous()), _ptr(ga), n,
                                           _stream()))
    return ga


def op_sqrtm_ns_backward_diag(root, grad_diag):
    """Lyapunov backward for grad_root = grad_diag * I (the plan's code path)."""
    lib = load_library()
    n = root.shape[-1]
    ga = torch.empty(root.shape, dtype=root.dtype, device=root.device)
    with torch.cuda.device(root.device):
        _check(lib.st_op_sqrtm_ns_backward_diag(_ptr(root.contiguous()), float(grad_diag), _ptr(ga), n, _stream()))
    return ga


def op_sqrtm_time(n, iters=20):
    """(forward, backward) microseconds per NS-12 chain, HIP events (tools/ns_bench.py)."""
    lib = load_library()
    f, b = ctypes.c_double(), ctypes.c_double()
    _check(lib.st_op_sqrtm_time(int(n), int(iters), ctypes.byref(f), ctypes.byref(b), _stream()))
    return f.value, b.value


def op_mfma_rate(lds_reads=0, waves=8, steps=20000, launches=10):
    """(TFLOP/s, shader MHz) the fp16 matrix pipe sustains under the XL convolution tile's consumer pattern with
    `lds_reads` ds_read_b128 per 12 MFMAs (csrc/st_diag.hip; tools/mfma_rate.py)."""
    lib = load_library()
    t, m = ctypes.c_double(), ctypes.c_double()
    _check(lib.st_op_mfma_rate(int(lds_reads), int(waves), int(steps), int(launches), ctypes.byref(t),
                               ctypes.byref(m), _stream()))
    return t.value, m.value


def op_mfma_valu_rate(lds_reads, waves, steps, valu_waves, valu_steps, valu_prio=0, launches=10):
    """(TFLOP/s, MHz, cycles per VALU instruction of the VALU-only waves, cycles per MFMA of an MFMA wave)."""
    lib = load_library()
    t, m = ctypes.c_double(), ctypes.c_double()
    c = (ctypes.c_double * 2)()
    _check(lib.st_op_mfma_valu_rate(int(lds_reads), int(waves), int(steps), int(launches), int(valu_waves),
                                    int(valu_steps), int(valu_prio), ctypes.byref(t), ctypes.byref(m), c, _stream()))
    return t.value, m.value, c[0], c[1]


def op_winograd_consumer_rate(steps=4096, launches=5):
    """TFLOP/s of MFMA work sustained in the Winograd tile's consumer pattern (csrc/st_diag.hip wino_rate_kernel)."""
    lib = load_library()
    t = ctypes.c_double()
    _check(lib.st_op_winograd_consumer_rate(int(steps), int(launches), ctypes.byref(t), _stream()))
    return t.value


def op_grid_barrier_time(workgroups=256, rounds=200, payload_floats=1024, groups=0):
    """(microseconds per round, stale reads) of device-wide barriers inside one launch (csrc/st_diag.hip)."""
    lib = load_library()
    us, err = ctypes.c_double(), ctypes.c_int()
    _check(lib.st_op_grid_barrier_time(int(workgroups), int(rounds), int(payload_floats), int(groups), ctypes.byref(us),
                                       ctypes.byref(err), _stream()))
    return us.value, err.value


def op_tv_loss(image):
    lib = load_library()
    h, w = image.shape[-2:]
    loss = torch.zeros(1, device=image.device, dtype=torch.float32)
    grad = torch.empty_like(image)
    with torch.cuda.device(image.device):
        _check(lib.st_op_tv_loss(_ptr(image.contiguous()), h, w, _ptr(loss), _ptr(grad), _stream()))
    return loss, grad


def term_scratch(device):
    """(scratch, ticket) for op_mse_term / op_tv_term: the reduction scratch and ONE zeroed ticket word, which every call leaves
    zero - calls on one stream may share the pair back to back."""
    return _reduce_scratch(device), torch.zeros(4, device=device, dtype=torch.int32)


def op_mse_term(x, target, weight=1.0, scratch=None, loss=None, grad=None):
    """The closure's one-launch content MSE (st_op_mse_term): (loss [1], grad) by the plan's own kernel, the value finished by
    the launch's last workgroup.  scratch: a ``term_scratch`` pair to share between calls; loss / grad: outputs to write into."""
    lib = load_library()
    partials, ticket = scratch if scratch is not None else term_scratch(x.device)
    loss = torch.zeros(1, device=x.device, dtype=torch.float32) if loss is None else loss
    grad = torch.empty_like(x) if grad is None else grad
    with torch.cuda.device(x.device):
        _check(lib.st_op_mse_term(_ptr(x), _ptr(target), x.numel(), float(weight), _ptr(partials), ctypes.c_void_p(ticket.data_ptr()), _ptr(loss),
                                  _ptr(grad), _stream()))
    return loss, grad


def op_tv_term(image, weight=1.0, scratch=None, loss=None, grad=None):
    """The closure's TV term (st_op_tv_term): (loss [1], grad) with the value finished by the border launch's last workgroup."""
    lib = load_library()
    h, w = image.shape[-2:]
    partials, ticket = scratch if scratch is not None else term_scratch(image.device)
    loss = torch.zeros(1, device=image.device, dtype=torch.float32) if loss is None else loss
    grad = torch.empty_like(image) if grad is None else grad
    with torch.cuda.device(image.device):
        _check(lib.st_op_tv_term(_ptr(image), h, w, float(weight), _ptr(partials), ctypes.c_void_p(ticket.data_ptr()), _ptr(loss), _ptr(grad), _stream()))
    return loss, grad


def op_conv3x3_time(cin, cout, height, width, dgrad=False, precision=4, iters=20):
    """Average microseconds per launch of the 3x3 convolution on device-resident random operands (st_op_conv3x3_time)."""
    lib = load_library()
    us = ctypes.c_double()
    _check(lib.st_op_conv3x3_time(int(cin), int(cout), int(height), int(width), 1 if dgrad else 0, int(precision), int(iters),
                                  ctypes.byref(us), _stream()))
    return us.value


def op_conv3x3(x, weight, bias, relu, precision=0):
    lib = load_library()
    cout, cin = weight.shape[:2]
    h, w = x.shape[-2:]
    out = torch.empty((1, cout, h, w), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_conv3x3(_ptr(x.contiguous()), _ptr(weight.contiguous()),
                                 _ptr(bias.contiguous()) if bias is not None else None, _ptr(out), cin, cout,
                                 h, w, 1 if relu else 0, int(precision), _stream()))
    return out


def op_conv3x3_strip(x, halo, has_up, has_down, weight, bias, relu, dgrad, precision=4):
    """The 3x3 convolution (or its data gradient) on a row strip: ``halo`` = [2, C, W] neighbour rows."""
    lib = load_library()
    cout, cin = weight.shape[:2]
    h, w = x.shape[-2:]
    out = torch.empty((1, cin if dgrad else cout, h, w), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_conv3x3_strip(_ptr(x.contiguous()), _ptr(halo.contiguous()), int(bool(has_up)),
                                       int(bool(has_down)), _ptr(weight.contiguous()),
                                       _ptr(bias.contiguous()) if bias is not None else None, _ptr(out), cin, cout,
                                       h, w, 1 if relu else 0, 1 if dgrad else 0, int(precision), _stream()))
    return out


def op_conv3x3_strip_ex(x, halo, has_up, has_down, weight, bias, relu, dgrad, out=None, out_mask=None, overlap=False,
                        precision=4):
    """op_conv3x3_strip with the plan's epilogue options: ``out`` given = accumulate into it (in place, returned),
    ``out_mask``, ``overlap`` = the interior + boundary two-launch form."""
    lib = load_library()
    cout, cin = weight.shape[:2]
    h, w = x.shape[-2:]
    acc = out is not None
    if out is None:
        out = torch.empty((1, cin if dgrad else cout, h, w), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_conv3x3_strip_ex(_ptr(x.contiguous()), _ptr(halo.contiguous()) if halo is not None else None, int(bool(has_up)),
                                          int(bool(has_down)), _ptr(weight.contiguous()),
                                          _ptr(bias.contiguous()) if bias is not None else None, _ptr(out),
                                          _ptr(out_mask.contiguous()) if out_mask is not None else None, cin, cout, h, w,
                                          1 if relu else 0, 1 if dgrad else 0, 1 if acc else 0, 1 if overlap else 0,
                                          int(precision), _stream()))
    return out


def op_conv1x1(x, weight, bias, precision=0):
    """x [Cin, npix], weight [Cout, Cin], bias [Cout] or None -> [Cout, npix] (the style heads' gradient step)."""
    lib = load_library()
    cout, cin = weight.shape
    npix = x.shape[1]
    out = torch.empty((cout, npix), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_conv1x1(_ptr(x.contiguous()), _ptr(weight.contiguous()),
                                 _ptr(bias.contiguous()) if bias is not None else None, _ptr(out), cin, cout,
                                 npix, int(precision), _stream()))
    return out


POOL_MODES = {'max': 0, 'average': 1, 'l2': 2}


def op_pool2x2(x, pooling, out=None):
    """x [C, H, W] -> [C, H // 2, W // 2] by the plan's pooling launcher; `pooling` in POOL_MODES.  `out` (optional, a
    contiguous fp32 tensor of that many elements) is written in place - the alignment of its pointer is the caller's."""
    lib = load_library()
    c, h, w = x.shape[-3:]
    if out is None:
        out = torch.empty((c, h // 2, w // 2), device=x.device, dtype=torch.float32)
    assert out.numel() == c * (h // 2) * (w // 2)
    with torch.cuda.device(x.device):
        _check(lib.st_op_pool2x2(_ptr(x.contiguous()), _ptr(out), c, h, w, POOL_MODES[pooling], _stream()))
    return out


def op_pool2x2_backward(x, grad_out, pooling, grad_in=None):
    """Gradient [C, H, W] of op_pool2x2(x) for grad_out [C, H // 2, W // 2], masked by (x > 0)."""
    lib = load_library()
    c, h, w = x.shape[-3:]
    assert grad_out.numel() == c * (h // 2) * (w // 2)
    if grad_in is None:
        grad_in = torch.empty((c, h, w), device=x.device, dtype=torch.float32)
    assert grad_in.numel() == c * h * w
    with torch.cuda.device(x.device):
        _check(lib.st_op_pool2x2_backward(_ptr(x.contiguous()), _ptr(grad_out.contiguous()), _ptr(grad_in), c, h, w,
                                          POOL_MODES[pooling], _stream()))
    return grad_in


def op_conv3x3_dgrad(grad_out, relu_out, weight, precision=0):
    lib = load_library()
    cout, cin = weight.shape[:2]
    h, w = grad_out.shape[-2:]
    gin = torch.empty((1, cin, h, w), device=grad_out.device, dtype=torch.float32)
    with torch.cuda.device(grad_out.device):
        _check(lib.st_op_conv3x3_dgrad(_ptr(grad_out.contiguous()),
                                       _ptr(relu_out.contiguous()) if relu_out is not None else None,
                                       _ptr(weight.contiguous()), _ptr(gin), cin, cout, h, w, int(precision),
                                       _stream()))
    return gin


# ---- the pointwise loss terms with a device-scalar upstream gradient (style_transfer/losses.py) -------------------------
def _reduce_scratch(device):
    """The per-call reduction scratch of the value entries (include/st_amd.h: the caller owns it)."""
    return torch.empty(int(load_library().st_op_reduce_scratch_floats()), device=device, dtype=torch.float32)


def op_mse_loss(x, target):
    """nn.MSELoss value as a 0-dim device tensor (st_op_mse_loss)."""
    lib = load_library()
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_mse_loss(_ptr(x), _ptr(target), x.numel(), _ptr(_reduce_scratch(x.device)), _ptr(loss), _stream()))
    return loss


def op_mse_loss_backward(x, target, upstream):
    lib = load_library()
    grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_mse_loss_backward(_ptr(x), _ptr(target), x.numel(), _ptr(upstream), _ptr(grad), _stream()))
    return grad


def op_scaled_mse_loss(x, target, eps):
    """(ScaledMSELoss value [0-dim], totals [2] = sum d^2, sum |d| + eps) - st_op_scaled_mse_loss."""
    lib = load_library()
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    totals = torch.empty(2, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_scaled_mse_loss(_ptr(x), _ptr(target), x.numel(), float(eps), _ptr(_reduce_scratch(x.device)),
                                         _ptr(totals), _ptr(loss), _stream()))
    return loss, totals


def op_scaled_mse_loss_backward(x, target, totals, upstream):
    lib = load_library()
    grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_scaled_mse_loss_backward(_ptr(x), _ptr(target), x.numel(), _ptr(totals), _ptr(upstream), _ptr(grad),
                                                  _stream()))
    return grad


def _channel_stats_scratch(x):
    c, npix = int(x.shape[-3]), int(x.shape[-2]) * int(x.shape[-1])
    floats = int(load_library().st_op_channel_stats_scratch_floats(c, npix))
    return c, npix, torch.empty(max(floats, 1), device=x.device, dtype=torch.float32)


def op_channel_moments(x):
    """(mean [C], the diagonal of the second raw moment [C]) over the pixels of a [..., C, H, W] tensor (one image) -
    st_op_channel_moments."""
    lib = load_library()
    c, npix, scratch = _channel_stats_scratch(x)
    mean = torch.empty(c, device=x.device, dtype=torch.float32)
    srm = torch.empty(c, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_channel_moments(_ptr(x), c, npix, _ptr(scratch), _ptr(mean), _ptr(srm), _stream()))
    return mean, srm


def op_w2_diag_loss(x, mean_t, std_t, eps):
    """(the diagonal W2 loss [0-dim], the gradient's coefficients [2 C]) - st_op_w2_diag_loss."""
    lib = load_library()
    c, npix, scratch = _channel_stats_scratch(x)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    coeffs = torch.empty(2 * c, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_w2_diag_loss(_ptr(x), c, npix, _ptr(mean_t), _ptr(std_t), float(eps), _ptr(scratch), _ptr(coeffs),
                                      _ptr(loss), _stream()))
    return loss, coeffs


def op_w2_diag_loss_backward(x, coeffs, upstream):
    lib = load_library()
    c, npix = int(x.shape[-3]), int(x.shape[-2]) * int(x.shape[-1])
    grad = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_w2_diag_loss_backward(_ptr(x), c, npix, _ptr(coeffs), _ptr(upstream), _ptr(grad), _stream()))
    return grad


def sort_chunk():
    """The keys one workgroup of the segmented sort orders in LDS (st_op_sort_chunk): rows up to this length need no merge pass."""
    return int(load_library().st_op_sort_chunk())


def gram_split_plan(channels, npix, precision='fp16x3'):
    """(splits, per_split, wide) of the Gram moments of a [channels, npix] tap as ``Head(..., precision).moments`` runs them
    (st_op_gram_split_plan; no device call): split s owns the pixels [s per_split, min((s + 1) per_split, npix))."""
    lib = load_library(require_gpu=False)
    splits, per_split, wide = ctypes.c_int(), ctypes.c_longlong(), ctypes.c_int()
    _check(lib.st_op_gram_split_plan(int(channels), int(npix), Net.PRECISIONS[precision], ctypes.byref(splits),
                                     ctypes.byref(per_split), ctypes.byref(wide)))
    return splits.value, per_split.value, bool(wide.value)


def _rows(x):
    """A [..., C, h, w] tensor (one image) or a [C, N] matrix as (C, N)."""
    if x.ndim == 2:
        return int(x.shape[0]), int(x.shape[1])
    return int(x.shape[-3]), int(x.shape[-2]) * int(x.shape[-1])


def _sort_scratch(x, c, n):
    nbytes = int(load_library().st_op_sort_scratch_bytes(c, n))
    return torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)


def op_channel_sort(x, values=True, indices=True):
    """(sorted rows [C, N] fp32, permutation [C, N] int64) of a [C, N] matrix or a [..., C, h, w] tensor (one image): per
    row the stable ascending order of ``x + 0.0`` (st_op_channel_sort).  An output not asked for is None."""
    lib = load_library()
    c, n = _rows(x)
    scratch = _sort_scratch(x, c, n)
    out = torch.empty((c, n), device=x.device, dtype=torch.float32) if values else None
    perm = torch.empty((c, n), device=x.device, dtype=torch.int32) if indices else None
    with torch.cuda.device(x.device):
        _check(lib.st_op_channel_sort(_ptr(x), c, n, ctypes.c_void_p(scratch.data_ptr()), _ptr(out),
                                      ctypes.c_void_p(perm.data_ptr()) if indices else None, _stream()))
    if indices:                                    # (uint32 indices: the bits of an int32 tensor, widened without sign)
        perm = perm.to(torch.int64) & 0xffffffff
    return out, perm


def op_resample_quantiles(q, n_out):
    """The quantile functions q [C, n_in] (sorted rows) at n_out midpoints, [C, n_out] (st_op_resample_quantiles)."""
    lib = load_library()
    c, n_in = int(q.shape[0]), int(q.shape[1])
    out = torch.empty((c, int(n_out)), device=q.device, dtype=torch.float32)
    with torch.cuda.device(q.device):
        _check(lib.st_op_resample_quantiles(_ptr(q), c, n_in, int(n_out), _ptr(out), _stream()))
    return out


def op_w2_marginal_loss(x, target):
    """(the marginal W2 loss [0-dim], its gradient at weight 1, shaped like x) - st_op_w2_marginal_loss; target [C, N]."""
    lib = load_library()
    c, n = _rows(x)
    scratch = _sort_scratch(x, c, n)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    unit = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_w2_marginal_loss(_ptr(x), c, n, _ptr(target), ctypes.c_void_p(scratch.data_ptr()), _ptr(unit), _ptr(loss),
                                          _stream()))
    return loss, unit


def op_w2_marginal_loss_backward(unit_grad, upstream):
    lib = load_library()
    grad = torch.empty(unit_grad.shape, device=unit_grad.device, dtype=torch.float32)
    with torch.cuda.device(unit_grad.device):
        _check(lib.st_op_w2_marginal_loss_backward(_ptr(unit_grad), unit_grad.numel(), _ptr(upstream), _ptr(grad), _stream()))
    return grad


def nearest_geometry():
    """(K chunk, pixel tile, k tile) of the nearest-neighbour search kernel (st_op_nearest_k_chunk / _pixel_tile / _k_tile)."""
    lib = load_library()
    return int(lib.st_op_nearest_k_chunk()), int(lib.st_op_nearest_pixel_tile()), int(lib.st_op_nearest_k_tile())


def nearest_splits(n, m):
    """The splits of the k range the search runs for n pixels against m style vectors (st_op_nearest_splits): by the shape alone."""
    return int(load_library().st_op_nearest_splits(int(n), int(m)))


def op_nearest_prepare(vectors):
    """The style set [C, M] as the search kernels read it (st_op_nearest_prepare): an opaque fp32 buffer for ``op_nearest_*``."""
    lib = load_library()
    c, m = int(vectors.shape[0]), int(vectors.shape[1])
    prepared = torch.empty(max(int(lib.st_op_nearest_prepared_floats(c, m)), 1), device=vectors.device, dtype=torch.float32)
    with torch.cuda.device(vectors.device):
        _check(lib.st_op_nearest_prepare(_ptr(vectors), c, m, _ptr(prepared), _stream()))
    return prepared


def _nearest_scratch(x, c, n, m):
    return torch.empty(max(int(load_library().st_op_nearest_scratch_floats(c, n, m)), 4), device=x.device, dtype=torch.float32)


def op_nearest_search(x, prepared, m):
    """(indices [N] int64, best scores [N] fp32) of a [C, N] matrix or a [..., C, h, w] tensor (one image) against a prepared
    set of m style vectors (st_op_nearest_search): ``argmax_k <f_i, s_k> - |s_k|^2 / 2``, ties to the lowest k."""
    lib = load_library()
    c, n = _rows(x)
    scratch = _nearest_scratch(x, c, n, m)
    idx = torch.empty((n,), device=x.device, dtype=torch.int32)
    score = torch.empty((n,), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_nearest_search(_ptr(x), c, n, _ptr(prepared), int(m), _ptr(scratch), ctypes.c_void_p(idx.data_ptr()),
                                        _ptr(score), _stream()))
    return idx.to(torch.int64), score


def op_nearest_loss(x, prepared, m):
    """(the nearest-neighbour loss [0-dim], its gradient at weight 1 shaped like x, the matches [N] int64) - st_op_nearest_loss."""
    lib = load_library()
    c, n = _rows(x)
    scratch = _nearest_scratch(x, c, n, m)
    idx = torch.empty((n,), device=x.device, dtype=torch.int32)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    unit = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_nearest_loss(_ptr(x), c, n, _ptr(prepared), int(m), _ptr(scratch), ctypes.c_void_p(idx.data_ptr()), _ptr(unit),
                                      _ptr(loss), _stream()))
    return loss, unit, idx.to(torch.int64)


def op_nearest_cosine_prepare(vectors, centered=False):
    """The style set [C, M] as the search and the cosine finish read it (st_op_nearest_cosine_prepare): unit rows, the bias
    ``-<mu, s^_k>`` and the centre ``mu`` (0, or with ``centered`` the set's mean) - an opaque fp32 buffer for
    ``op_nearest_cosine_loss`` and ``op_nearest_search``."""
    lib = load_library()
    c, m = int(vectors.shape[0]), int(vectors.shape[1])
    prepared = torch.empty(max(int(lib.st_op_nearest_cosine_prepared_floats(c, m)), 1), device=vectors.device, dtype=torch.float32)
    with torch.cuda.device(vectors.device):
        _check(lib.st_op_nearest_cosine_prepare(_ptr(vectors), c, m, int(centered), _ptr(prepared), _stream()))
    return prepared


def op_nearest_cosine_loss(x, prepared, m):
    """(the cosine nearest-neighbour loss [0-dim], its gradient at weight 1 shaped like x, the matches [N] int64) -
    st_op_nearest_cosine_loss."""
    lib = load_library()
    c, n = _rows(x)
    scratch = torch.empty(max(int(lib.st_op_nearest_cosine_scratch_floats(c, n, m)), 4), device=x.device, dtype=torch.float32)
    idx = torch.empty((n,), device=x.device, dtype=torch.int32)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    unit = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_nearest_cosine_loss(_ptr(x), c, n, _ptr(prepared), int(m), _ptr(scratch), ctypes.c_void_p(idx.data_ptr()),
                                             _ptr(unit), _ptr(loss), _stream()))
    return loss, unit, idx.to(torch.int64)


def op_nearest_loss_backward(unit_grad, upstream):
    lib = load_library()
    grad = torch.empty(unit_grad.shape, device=unit_grad.device, dtype=torch.float32)
    with torch.cuda.device(unit_grad.device):
        _check(lib.st_op_nearest_loss_backward(_ptr(unit_grad), unit_grad.numel(), _ptr(upstream), _ptr(grad), _stream()))
    return grad


def op_sliced_directions(seed, entry, epoch, projections, channels, device='cuda'):
    """(R [P, C], R^T [C, P]): P unit directions of (seed, entry, epoch) from the device generator (st_op_sliced_directions)."""
    lib = load_library()
    device = torch.device(device)
    r = torch.empty((int(projections), int(channels)), device=device, dtype=torch.float32)
    rt = torch.empty((int(channels), int(projections)), device=device, dtype=torch.float32)
    with torch.cuda.device(device):
        _check(lib.st_op_sliced_directions(int(seed) & 0xffffffffffffffff, int(entry), int(epoch) & 0xffffffffffffffff, int(projections),
                                           int(channels), _ptr(r), _ptr(rt), _stream()))
    return r, rt


def _sliced_scratch(x, c, p, n):
    nbytes = int(load_library().st_op_sliced_scratch_bytes(c, p, n))
    return torch.empty(max(nbytes, 16), device=x.device, dtype=torch.uint8)


def op_sliced_target(vectors, r, rt, n_out, target=None, weight=1.0):
    """One style image's share of a sliced target (st_op_sliced_target): ``weight`` times the quantile functions of the rows of
    ``r @ vectors`` ([C, M] -> [P, M]) at n_out midpoints, written to a new [P, n_out] tensor or, with ``target``, added onto it."""
    lib = load_library()
    c, m = int(vectors.shape[0]), int(vectors.shape[1])
    p = int(r.shape[0])
    scratch = _sliced_scratch(vectors, c, p, max(m, int(n_out)))
    accumulate = target is not None
    if target is None:
        target = torch.empty((p, int(n_out)), device=vectors.device, dtype=torch.float32)
    with torch.cuda.device(vectors.device):
        _check(lib.st_op_sliced_target(_ptr(vectors), c, m, _ptr(r), _ptr(rt), p, int(n_out), ctypes.c_void_p(scratch.data_ptr()),
                                       _ptr(target), int(accumulate), float(weight), _stream()))
    return target


def op_sliced_project(x, r, rt):
    """Y [P, N] = r @ x as ``op_sliced_loss`` computes and sorts it, bit for bit (st_op_sliced_project)."""
    lib = load_library()
    c, n = _rows(x)
    p = int(r.shape[0])
    scratch = _sliced_scratch(x, c, p, n)
    y = torch.empty((p, n), device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_sliced_project(_ptr(x), c, n, _ptr(r), _ptr(rt), p, ctypes.c_void_p(scratch.data_ptr()), _ptr(y), _stream()))
    return y


def op_sliced_loss(x, r, rt, target):
    """(the sliced Wasserstein loss [0-dim], its gradient at weight 1, shaped like x) - st_op_sliced_loss; x a [C, N] matrix or a
    [..., C, h, w] tensor (one image), r [P, C], rt [C, P], target [P, N]."""
    lib = load_library()
    c, n = _rows(x)
    p = int(r.shape[0])
    scratch = _sliced_scratch(x, c, p, n)
    loss = torch.empty((), device=x.device, dtype=torch.float32)
    unit = torch.empty(x.shape, device=x.device, dtype=torch.float32)
    with torch.cuda.device(x.device):
        _check(lib.st_op_sliced_loss(_ptr(x), c, n, _ptr(r), _ptr(rt), p, _ptr(target), ctypes.c_void_p(scratch.data_ptr()), _ptr(unit),
                                     _ptr(loss), _stream()))
    return loss, unit


def op_sliced_loss_backward(unit_grad, upstream):
    lib = load_library()
    grad = torch.empty(unit_grad.shape, device=unit_grad.device, dtype=torch.float32)
    with torch.cuda.device(unit_grad.device):
        _check(lib.st_op_sliced_loss_backward(_ptr(unit_grad), unit_grad.numel(), _ptr(upstream), _ptr(grad), _stream()))
    return grad


def op_tv_value(image):
    """TVLoss value of a [..., 3, H, W] image (one image) as a 0-dim device tensor (st_op_tv_value)."""
    lib = load_library()
    h, w = image.shape[-2:]
    loss = torch.empty((), device=image.device, dtype=torch.float32)
    with torch.cuda.device(image.device):
        _check(lib.st_op_tv_value(_ptr(image), h, w, _ptr(_reduce_scratch(image.device)), _ptr(loss), _stream()))
    return loss


def op_tv_loss_backward(image, upstream):
    lib = load_library()
    h, w = image.shape[-2:]
    grad = torch.empty(image.shape, device=image.device, dtype=torch.float32)
    with torch.cuda.device(image.device):
        _check(lib.st_op_tv_loss_backward(_ptr(image), h, w, _ptr(upstream), _ptr(grad), _stream()))
    return grad


def _laplacian_shape(image, pool):
    c, h, w = image.shape[-3:]
    return int(c), int(h), int(w), int(pool)


def op_laplacian_target(image, pool):
    """``L(avg_pool2d(image, pool))`` of a [..., C, H, W] image (one image) as a [C, H // pool, W // pool] device tensor
    (st_op_laplacian_target): the 4-neighbour Laplacian on the replicate-padded pooled map."""
    lib = load_library()
    c, h, w, pool = _laplacian_shape(image, pool)
    target = torch.empty((c, h // pool, w // pool), device=image.device, dtype=torch.float32)
    scratch = torch.empty(max(int(lib.st_op_laplacian_scratch_floats(c, h, w, pool)), 1), device=image.device, dtype=torch.float32)
    with torch.cuda.device(image.device):
        _check(lib.st_op_laplacian_target(_ptr(image), c, h, w, pool, _ptr(scratch), _ptr(target), _stream()))
    return target


def op_laplacian_value(image, target, pool):
    """(mean((L(avg_pool2d(image, pool)) - target) ** 2) [0-dim], the residual [C, h, w]) - st_op_laplacian_value."""
    lib = load_library()
    c, h, w, pool = _laplacian_shape(image, pool)
    loss = torch.empty((), device=image.device, dtype=torch.float32)
    residual = torch.empty((c, h // pool, w // pool), device=image.device, dtype=torch.float32)
    scratch = torch.empty(max(int(lib.st_op_laplacian_scratch_floats(c, h, w, pool)), 1), device=image.device, dtype=torch.float32)
    with torch.cuda.device(image.device):
        _check(lib.st_op_laplacian_value(_ptr(image), _ptr(target), c, h, w, pool, _ptr(scratch), _ptr(residual), _ptr(loss), _stream()))
    return loss, residual


def op_laplacian_backward(residual, shape, pool, upstream):
    """The gradient of ``op_laplacian_value`` times the device scalar ``upstream``, as a tensor of the image's ``shape``
    (st_op_laplacian_backward)."""
    lib = load_library()
    c, h, w = (int(d) for d in shape[-3:])
    grad = torch.empty(tuple(shape), device=residual.device, dtype=torch.float32)
    with torch.cuda.device(residual.device):
        _check(lib.st_op_laplacian_backward(_ptr(residual), c, h, w, int(pool), _ptr(upstream), _ptr(grad), _stream()))
    return grad
