"""The memory around every caller-owned buffer of the C ABI, and the pointers a caller may legally pass off alignment.

Every other GPU test allocates its outputs and scratch with torch.empty - exactly sized, 512-byte aligned by the caching
allocator, with slack behind - so a kernel that stores a few elements past its output, uses more scratch than the size
function promises, reads garbage past an input and multiplies it by a zero mask, or mishandles a pointer that is dense fp32
but not 16-byte aligned (`batch[1]` of a [2, 3, 45, 54] tensor) cannot be seen.  Here the test owns every buffer
(tests/fences.py): 64 KiB of a recognisable quiet NaN in front of and behind each payload, outputs pre-filled with it,
scratch of exactly the promised bytes filled with 0xFF, and every pointer run at offsets of 0 to 3 floats from a 16-byte
boundary - inputs shifted, outputs shifted, both.  The C ABI is called through ctypes, never through the allocating wrappers.

Each case asserts: the return code (0, or the documented refusal that writes nothing); fences intact and every output element
written; nothing non-finite in an output (poison read from beyond an input shows up here); parity with the float64 reference
of the entry's existing test at that test's bar (named at each entry); selections and permutations equal to the offset-0 run
exactly; a second call on the same buffers, scratch as the first call left it, giving the same bits.  The difference between
a shifted and the offset-0 result is printed as an observation (a scalar path may add in another order); profiles/caller_buffers.md
records what was seen.
"""
import ctypes
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import fences as F
from conftest import rel_l2
import st_oracle as O

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP = 2.0 ** -23
UPSTREAM = 0.37


def _hip():
    from style_transfer import _hip
    return _hip


def _lib():
    return _hip().load_library()


def _stream():
    return _hip()._stream()


def _last_error():
    return _lib().st_last_error().decode('utf-8', 'replace')


# the offsets (floats past a 16-byte boundary) of a vector-eligible shape: aligned; inputs shifted; outputs shifted; both
SHIFTS = [(0, 0)] + [pair for k in (1, 2, 3) for pair in ((k, 0), (0, k), (k, k))]
RAGGED_SHIFTS = [(0, 0), (1, 2)]          # a shape that never takes a 16-byte path: aligned, and everything shifted once


class Buffers:
    """The fenced buffers of one call: inputs (payload copied in), outputs (payload poisoned) and scratch (0xFF)."""

    def __init__(self):
        self.items = {}

    def inp(self, name, tensor, offset=0):
        view, whole = F.fenced_input(tensor.to(DEV), offset)
        self.items[name] = ('in', view, whole)
        return ctypes.c_void_p(view.data_ptr())

    def out(self, name, n, offset=0, dtype=torch.float32):
        view, whole = F.fenced(n, dtype, offset, DEV)
        self.items[name] = ('out', view, whole)
        return ctypes.c_void_p(view.data_ptr())

    def inout(self, name, tensor, offset=0):
        view, whole = F.fenced_input(tensor.to(DEV), offset)
        self.items[name] = ('inout', view, whole)
        return ctypes.c_void_p(view.data_ptr())

    def opaque(self, name, n, offset=0):
        """A poisoned buffer the entry owns the layout of (a head's state): fences and repeatability, no 'every element'."""
        view, whole = F.fenced(n, torch.float32, offset, DEV)
        self.items[name] = ('inout', view, whole)
        return ctypes.c_void_p(view.data_ptr())

    def scratch(self, name, nbytes, align=4, offset_bytes=0):
        view, whole = F.fenced_scratch(nbytes, align, offset_bytes, DEV)
        self.items[name] = ('scratch', view, whole)
        return ctypes.c_void_p(view.data_ptr() if nbytes else whole.data_ptr() + F.FENCE_BYTES + 256)

    def ptr(self, name):
        return ctypes.c_void_p(self.items[name][1].data_ptr())

    def get(self, name):
        return self.items[name][1].detach().cpu().clone()

    def verify(self, tag, written=None):
        """Fences intact everywhere; every output named in `written` (default: all) fully written and finite."""
        _sync()
        found = []
        for name, (role, view, whole) in self.items.items():
            is_out = role == 'out' and (written is None or name in written)
            try:
                F.check_view(whole, view, written=is_out, name=f'{tag}: {name}')
            except F.FenceError as e:
                found.append(str(e))
            if is_out and view.is_floating_point() and not bool(torch.isfinite(view).all()):
                bad = (~torch.isfinite(view)).nonzero().flatten()[:8].tolist()
                found.append(f'{tag}: {name}: non-finite output element(s), first at {bad}')
        assert not found, '\n'.join(found)

    def bits(self, names=None):
        """The payload bits of the outputs (and in/out buffers), for 'the same bits' comparisons."""
        _sync()
        return {name: F.snapshot(view) for name, (role, view, whole) in self.items.items()
                if role in ('out', 'inout') and (names is None or name in names)}

    def everything(self):
        _sync()
        return {name: F.snapshot(whole) for name, (role, view, whole) in self.items.items()}


def _same_bits(tag, a, b):
    for name in a:
        assert torch.equal(a[name], b[name]), f'{tag}: {name}: a second call on the same buffers gave other bits'


def _sync(tag=''):
    """Wait for the device.  A HIP runtime error here is a GPU fault: nothing more is started on the device in this session."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f'{tag}: the device reported {e}: stopping the session, no further GPU work', returncode=3)


def _ok(rc, tag):
    if rc != 0 and any(word in _last_error().lower() for word in ('illegal', 'fault', 'launch failure', 'unspecified')):
        pytest.exit(f'{tag}: rc {rc}: {_last_error()}: stopping the session, no further GPU work', returncode=3)
    assert rc == 0, f'{tag}: rc {rc}: {_last_error()}'


OBSERVED = {}


def _observe(entry, case, shift, got, base):
    """Print (and keep) the largest difference between a shifted run and the offset-0 run of the same case."""
    worst = 0.0
    for name in got:
        if got[name].is_floating_point() and got[name].numel():
            scale = float(base[name].double().abs().max())
            worst = max(worst, float((got[name].double() - base[name].double()).abs().max()) / (scale if scale > 0 else 1.0))
    key = (entry, str(case))
    OBSERVED[key] = max(OBSERVED.get(key, 0.0), worst)
    print(f'[caller-buffers] {entry} {case} shift {shift}: max |difference from offset 0| / max |value| {worst:.2e}')


def _rel(got, want):
    want = float(want)
    return abs(float(got) - want) / abs(want) if want != 0 else abs(float(got))


def _gerr(got, want):
    want = torch.as_tensor(want).double().reshape(-1)
    got = got.double().reshape(-1)
    return rel_l2(got, want) if float(want.norm()) > 0 else float(got.norm())


# =====================================================================================================================
# 0. the detector fires on the device
# =====================================================================================================================
def test_positive_control_the_detector_fires_on_the_device():
    """st_op_mse_loss_backward with `count` four larger than the fenced payload: the four extra elements lie inside the
    test's own allocation (64 KiB of fence), so nothing outside it is touched - and `check` must report the broken fence."""
    lib, n = _lib(), 4096
    g = torch.Generator().manual_seed(1)
    b = Buffers()
    x = b.inp('x', torch.randn(n + 4, generator=g))
    t = b.inp('t', torch.randn(n + 4, generator=g))
    up = b.inp('upstream', torch.tensor([1.0]))
    grad = b.out('grad', n)
    _ok(lib.st_op_mse_loss_backward(x, t, n + 4, up, grad, _stream()), 'positive control')
    _sync()
    kind, view, whole = b.items['grad']
    found = F.problems(whole, 0, n)
    assert len(found) == 1 and '4 element(s) written AFTER the payload, first at [4096, 4097, 4098, 4099]' in found[0], found
    with pytest.raises(AssertionError, match='AFTER the payload'):
        b.verify('positive control')
    # and an element never written, on the device: count four SMALLER than the payload
    b2 = Buffers()
    grad2 = b2.out('grad', n)
    _ok(lib.st_op_mse_loss_backward(x, t, n - 4, up, grad2, _stream()), 'positive control')
    with pytest.raises(AssertionError, match='4 of 4096 output element'):
        b2.verify('positive control')


# =====================================================================================================================
# 1. mse / scaled mse (csrc/st_head.hip diff_sums, diff_grad: vec4 = count % 4 == 0 and x, target (, grad) 16-byte aligned)
#    reference and bars: tests/test_native_losses_gpu.py - the float64 formula, value and gradient 1e-4
# =====================================================================================================================
POINTWISE_COUNTS = [1, 1023, 4096, 64 * 2430]
# (x, target, outputs / totals): the three are shifted independently
POINTWISE_SHIFTS = [(0, 0, 0)] + [s for k in (1, 2, 3) for s in ((k, k, 0), (0, 0, k), (k, k, k))] + [(1, 0, 0), (0, 2, 0), (1, 3, 2)]
POINTWISE_BAR = 1e-4


def _pointwise_run(kind, x, t, shift):
    lib, n = _lib(), x.numel()
    sx, st, so = shift
    tag = f'{kind} count {n} shift {shift}'
    b = Buffers()
    px, pt = b.inp('x', x, sx), b.inp('t', t, st)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    scratch = b.scratch('scratch', 4 * int(lib.st_op_reduce_scratch_floats()), 16, 4 * so)
    loss, grad = b.out('loss', 1, so), b.out('grad', n, so)
    if kind == 'mse':
        def call():
            _ok(lib.st_op_mse_loss(px, pt, n, scratch, loss, _stream()), tag)
            _ok(lib.st_op_mse_loss_backward(px, pt, n, up, grad, _stream()), tag)
    else:
        totals = b.out('totals', 2, so)

        def call():
            _ok(lib.st_op_scaled_mse_loss(px, pt, n, 1e-8, scratch, totals, loss, _stream()), tag)
            _ok(lib.st_op_scaled_mse_loss_backward(px, pt, n, totals, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('count', POINTWISE_COUNTS)
@pytest.mark.parametrize('kind', ['mse', 'scaled_mse'])
def test_mse_and_scaled_mse(kind, count):
    g = torch.Generator().manual_seed(count)
    x, t = torch.randn(count, generator=g), 1.3 * torch.randn(count, generator=g) + 0.2
    d = x.double() - t.double()
    if kind == 'mse':
        want = float((d * d).mean())
        want_grad = UPSTREAM * 2 * d / count
    else:
        s2, s1 = float((d * d).sum()), float(d.abs().sum()) + 1e-8
        want = s2 / s1
        want_grad = UPSTREAM * (2 * d - want * torch.sign(d)) / s1
    base = None
    for shift in (POINTWISE_SHIFTS if count % 4 == 0 else [(0, 0, 0), (1, 3, 2)]):
        got = _pointwise_run(kind, x, t, shift)
        ev, eg = _rel(got['loss'][0], want), _gerr(got['grad'], want_grad)
        assert ev <= POINTWISE_BAR and eg <= POINTWISE_BAR, (kind, count, shift, ev, eg)
        if kind == 'scaled_mse':
            assert _rel(got['totals'][0], s2) <= POINTWISE_BAR and _rel(got['totals'][1], s1) <= POINTWISE_BAR
        base = base or got
        _observe(f'st_op_{kind}_loss(_backward)', count, shift, got, base)


# =====================================================================================================================
# 2. TV (csrc/st_pointwise.hip launch_tv_kernels: vec = W % 4 == 0, W >= 8, H >= 2, image and grad 16-byte aligned;
#    csrc/st_head.hip tv_value_kernel / tv_grad_kernel: scalar)
#    reference and bars: tests/test_kernels_gpu.py test_tv_loss_and_gradient - the oracle's TV, value and gradient 2e-6
#    (st_op_tv_loss); tests/test_native_losses_gpu.py - float64, 1e-4 (st_op_tv_value / st_op_tv_loss_backward)
# =====================================================================================================================
TV_SIZES = [(9, 12), (16, 16), (17, 300), (8, 4), (1, 8), (9, 13)]


def _tv_vector_eligible(h, w):
    return w % 4 == 0 and w >= 8 and h >= 2


def _tv_run(img, shift):
    lib = _lib()
    h, w = img.shape[-2:]
    si, so = shift
    tag = f'tv {h}x{w} shift {shift}'
    b = Buffers()
    pi = b.inp('image', img, si)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    scratch = b.scratch('scratch', 4 * int(lib.st_op_reduce_scratch_floats()), 16, 4 * so)
    loss, grad = b.out('loss', 1, so), b.out('grad', 3 * h * w, so)
    value, grad_up = b.out('value', 1, so), b.out('grad_up', 3 * h * w, so)

    def call():
        _ok(lib.st_op_tv_loss(pi, h, w, loss, grad, _stream()), tag)
        _ok(lib.st_op_tv_value(pi, h, w, scratch, value, _stream()), tag)
        _ok(lib.st_op_tv_loss_backward(pi, h, w, up, grad_up, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('size', TV_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_tv(size):
    h, w = size
    img = torch.rand((1, 3, h, w), generator=torch.Generator().manual_seed(h * 1000 + w))
    want_loss, want_grad = O.tv_loss_grad_closed_form(img)
    v64, g64 = O.tv_loss_grad_closed_form(img.double())
    base = None
    for shift in (SHIFTS if _tv_vector_eligible(h, w) else RAGGED_SHIFTS):
        got = _tv_run(img, shift)
        assert _rel(got['loss'][0], want_loss) < 2e-6, (size, shift)
        assert _gerr(got['grad'], want_grad) <= 2e-6, (size, shift)
        assert _rel(got['value'][0], v64) <= 1e-4 and _gerr(got['grad_up'], UPSTREAM * g64) <= 1e-4, (size, shift)
        base = base or got
        _observe('st_op_tv_loss / _value / _loss_backward', size, shift, got, base)


# =====================================================================================================================
# 3. the diagonal W2 entries (csrc/st_w2diag.hip launch_channel_stats: vec = npix % 4 == 0 and feat aligned;
#    launch_channel_affine_grad: ... and grad aligned; channel_stats_splits(npix) > 1 past one split's pixels)
#    reference and bars: tests/test_w2_diagonal_gpu.py test_the_operators_alone - test_w2_diagonal_cpu.formula64 in float64,
#    moments 1e-6 of the largest, value and gradient 1e-4
# =====================================================================================================================
def _stats_splits(c, npix):
    return (int(_lib().st_op_channel_stats_scratch_floats(c, npix)) - 4) // (2 * c)


def _first_split_npix():
    lo, hi = 1, 1 << 20
    assert _stats_splits(1, lo) == 1 and _stats_splits(1, hi) > 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if _stats_splits(1, mid) == 1 else (lo, mid)
    return hi


def _diag_run(x, mean_t, std_t, eps, shift):
    lib = _lib()
    c, npix = x.shape
    si, so = shift
    tag = f'w2diag C {c} npix {npix} shift {shift}'
    b = Buffers()
    feat = b.inp('feat', x, si)
    mt, st = b.inp('mean_t', mean_t, si), b.inp('std_t', std_t, si)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    nbytes = 4 * int(lib.st_op_channel_stats_scratch_floats(c, npix))
    s1, s2 = b.scratch('scratch moments', nbytes, 16, 4 * so), b.scratch('scratch loss', nbytes, 16, 4 * so)
    mean, srm = b.out('mean', c, so), b.out('srm', c, so)
    coeffs, loss, grad = b.out('coeffs', 2 * c, so), b.out('loss', 1, so), b.out('grad', c * npix, so)

    def call():
        _ok(lib.st_op_channel_moments(feat, c, npix, s1, mean, srm, _stream()), tag)
        _ok(lib.st_op_w2_diag_loss(feat, c, npix, mt, st, eps, s2, coeffs, loss, _stream()), tag)
        _ok(lib.st_op_w2_diag_loss_backward(feat, c, npix, coeffs, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('c', [1, 3, 64, 513])
def test_channel_moments_and_w2_diag(c):
    from test_w2_diagonal_cpu import formula64
    first_split = _first_split_npix()
    eps = 1e-4
    for npix in (1, 2430, 2432, first_split - 1, first_split, (first_split + 3) // 4 * 4 + 4):
        assert (_stats_splits(c, npix) > 1) == (npix >= first_split)
        g = torch.Generator().manual_seed(c * 100 + npix)
        x = (torch.randn((c, npix), generator=g) * (0.5 + torch.rand((c, 1), generator=g)) + torch.randn((c, 1), generator=g)).clamp(min=-0.3)
        t = torch.randn((c, npix + 5), generator=g) * 0.8 + 0.3
        x64, t64 = x.double().numpy(), t.double().numpy()
        mean_t = t64.mean(1)
        std_t = np.sqrt(np.maximum((t64 * t64).mean(1) - mean_t ** 2, 0) + eps)
        want_mean, want_srm = x64.mean(1), (x64 * x64).mean(1)
        want, want_grad = formula64(x64, mean_t, std_t, eps)
        base = None
        for shift in (SHIFTS if npix % 4 == 0 else RAGGED_SHIFTS):
            got = _diag_run(x, torch.from_numpy(mean_t).float(), torch.from_numpy(std_t).float(), eps, shift)
            em = float(np.abs(got['mean'].double().numpy() - want_mean).max() / max(np.abs(want_mean).max(), 1e-30))
            es = float(np.abs(got['srm'].double().numpy() - want_srm).max() / max(np.abs(want_srm).max(), 1e-30))
            ev, eg = _rel(got['loss'][0], want), _gerr(got['grad'], UPSTREAM * want_grad)
            assert em <= 1e-6 and es <= 1e-6, (c, npix, shift, em, es)
            assert ev <= 1e-4 and eg <= 1e-4, (c, npix, shift, ev, eg)
            base = base or got
            _observe('st_op_channel_moments / w2_diag_loss(_backward)', (c, npix), shift, got, base)


# =====================================================================================================================
# 4. the segmented sort, the resample and the marginal W2 entries (csrc/st_sort.hip: no alignment branch on feat; one LDS chunk
#    of st_op_sort_chunk() keys and merge passes beyond; `scratch` 256-byte aligned - u64 keys behind a header)
#    reference and bars: tests/test_w2_marginal_gpu.py - torch.sort(x + 0.0, stable=True) exactly; resample 1e-6 of max |q|;
#    marginal_formula in float64, value and gradient 1e-4
# =====================================================================================================================
def _sort_shapes():
    k = int(_lib().st_op_sort_chunk())
    return [(1, 1), (3, k), (3, k + 1), (2, 5 * k - 3), (513, 100)]


def _marginal_run(x, q, shift):
    lib = _lib()
    c, n = x.shape
    n_q = q.shape[1]
    si, so = shift
    tag = f'sort / marginal ({c}, {n}) shift {shift}'
    b = Buffers()
    feat, pq = b.inp('feat', x, si), b.inp('q', q, si)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    nbytes = int(lib.st_op_sort_scratch_bytes(c, n))
    s1, s2 = b.scratch('scratch sort', nbytes, 256), b.scratch('scratch loss', nbytes, 256)
    values, perm = b.out('values', c * n, so), b.out('perm', c * n, so, torch.int32)
    target, unit = b.out('target', c * n, so), b.out('unit', c * n, so)
    loss, grad = b.out('loss', 1, so), b.out('grad', c * n, so)

    def call():
        _ok(lib.st_op_channel_sort(feat, c, n, s1, values, perm, _stream()), tag)
        _ok(lib.st_op_resample_quantiles(pq, c, n_q, n, target, _stream()), tag)
        _ok(lib.st_op_w2_marginal_loss(feat, c, n, target, s2, unit, loss, _stream()), tag)
        _ok(lib.st_op_w2_marginal_loss_backward(unit, c * n, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('index', range(5))
def test_sort_resample_and_marginal(index):
    from test_w2_marginal_cpu import marginal_formula
    c, n = _sort_shapes()[index]
    g = torch.Generator().manual_seed(31 + index)
    x = (torch.randn((c, n), generator=g).clamp(min=0) * 1.5 - 0.1).contiguous()      # about half ties: the stable order is tested
    n_q = max(1, (n * 3) // 4 + 1)
    q = torch.sort(torch.randn((c, n_q), generator=g).clamp(min=0), dim=1).values.contiguous()
    want_sort = torch.sort(x + 0.0, dim=1, stable=True)
    want, want_grad = marginal_formula(x.double().numpy(), q.double().numpy())
    base = None
    for shift in (SHIFTS if n % 4 == 0 else RAGGED_SHIFTS):
        got = _marginal_run(x, q, shift)
        assert torch.equal(got['values'].view(c, n), want_sort.values), (c, n, shift)
        assert torch.equal(got['perm'].view(c, n).to(torch.int64) & 0xffffffff, want_sort.indices), (c, n, shift)
        ev, eg = _rel(got['loss'][0], want), _gerr(got['grad'], UPSTREAM * want_grad)
        assert ev <= 1e-4 and eg <= 1e-4, (c, n, shift, ev, eg)
        base = base or got
        assert torch.equal(got['perm'], base['perm']) and torch.equal(got['values'], base['values'])
        _observe('st_op_channel_sort / resample / w2_marginal_loss(_backward)', (c, n), shift, got, base)


@pytest.mark.parametrize('c, n_in, n_out', [(3, 1000, 1023), (3, 1000, 1024), (3, 1000, 1025), (2, 1025, 1000), (5, 1024, 2052),
                                            (3, 1000, 1000)])
def test_resample_on_both_sides_of_a_tile(c, n_in, n_out):
    """resample_rows_kernel owns 1024 elements of an output row per workgroup; n_in == n_out is a device-to-device copy."""
    from test_w2_marginal_cpu import resample_formula
    lib = _lib()
    q = torch.sort(torch.randn((c, n_in), generator=torch.Generator().manual_seed(n_in + n_out)).clamp(min=-0.5), dim=1).values.contiguous()
    want = resample_formula(q.double().numpy(), n_out)
    base = None
    for shift in (SHIFTS if n_out % 4 == 0 and n_in % 4 == 0 else RAGGED_SHIFTS + [(3, 1)]):
        tag = f'resample ({c}, {n_in}) -> {n_out} shift {shift}'
        b = Buffers()
        pq, out = b.inp('q', q, shift[0]), b.out('out', c * n_out, shift[1])
        for _ in range(2):
            _ok(lib.st_op_resample_quantiles(pq, c, n_in, n_out, out, _stream()), tag)
            b.verify(tag)
        got = b.get('out').view(c, n_out)
        if n_in == n_out:
            assert torch.equal(got, q)
        worst = float(np.abs(got.double().numpy() - want).max()) / float(q.abs().max())
        assert worst <= 1e-6 and _gerr(got, want) <= 1e-6, (tag, worst)
        base = got if base is None else base
        assert torch.equal(got, base), tag


def _refused(tag, rc, word, buffers, before):
    assert rc != 0, f'{tag}: a misaligned pointer the header forbids was accepted'
    # the argument at fault is the one named: "...: feat must be ...", "...: the state buffer must be ..."
    assert re.search(rf'(: |: the ){word}( buffer)? must be \d+-byte aligned', _last_error()), (tag, word, _last_error())
    after = buffers.everything()
    for name in before:
        assert torch.equal(before[name], after[name]), f'{tag}: {name} changed although the call was refused'


@pytest.mark.parametrize('offset_bytes', [4, 8, 16, 128])
def test_sort_and_marginal_refuse_a_misaligned_scratch(offset_bytes):
    lib, (c, n) = _lib(), (3, 100)
    x = torch.randn((c, n), generator=torch.Generator().manual_seed(5))
    b = Buffers()
    feat, target = b.inp('feat', x), b.inp('target', torch.sort(x, dim=1).values.contiguous())
    scratch = b.scratch('scratch', int(lib.st_op_sort_scratch_bytes(c, n)), 256, offset_bytes)
    values, perm, unit, loss = b.out('values', c * n), b.out('perm', c * n, 0, torch.int32), b.out('unit', c * n), b.out('loss', 1)
    before = b.everything()
    _refused('st_op_channel_sort', lib.st_op_channel_sort(feat, c, n, scratch, values, perm, _stream()), 'scratch', b, before)
    _refused('st_op_w2_marginal_loss', lib.st_op_w2_marginal_loss(feat, c, n, target, scratch, unit, loss, _stream()), 'scratch', b, before)


# =====================================================================================================================
# 5. the nearest-neighbour entries (csrc/st_nearest.hip launch_nearest_search: vec_ok = n % 4 == 0 and feat aligned; 128-pixel
#    and 128-vector tiles, M padded; splits of the k range; `prepared` and `scratch` 256-byte aligned)
#    reference and bars: tests/test_style_nearest_gpu.py - the float64 arg-min exactly on unrelated data, the header's deficit
#    bound, value and gradient 1e-4 against the float64 formula at the matches found
# =====================================================================================================================
def _nearest_shapes():
    lib = _lib()
    tpx, tk = int(lib.st_op_nearest_pixel_tile()), int(lib.st_op_nearest_k_tile())
    split = 4 * tk
    shapes = [(1, 1), (tpx - 1, tk - 1), (tpx, tk), (tpx + 1, tk + 1), (tpx + 4, split + 1), (2 * tpx, 2 * split + 1)]
    assert [int(lib.st_op_nearest_splits(n, m)) for n, m in shapes] == [1, 1, 1, 1, 2, 3]
    return shapes


def _nearest_run(f, s, shift):
    lib = _lib()
    (c, n), m = f.shape, s.shape[1]
    si, so = shift
    tag = f'nearest ({c}, {n}, {m}) shift {shift}'
    b = Buffers()
    feat, vectors = b.inp('feat', f, si), b.inp('vectors', s, si)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    prepared = b.scratch('prepared', 4 * int(lib.st_op_nearest_prepared_floats(c, m)), 256)
    nbytes = 4 * int(lib.st_op_nearest_scratch_floats(c, n, m))
    s1, s2 = b.scratch('scratch search', nbytes, 256), b.scratch('scratch loss', nbytes, 256)
    idx, score = b.out('idx', n, so, torch.int32), b.out('score', n, so)
    idx2, unit, loss, grad = b.out('idx loss', n, so, torch.int32), b.out('unit', c * n, so), b.out('loss', 1, so), b.out('grad', c * n, so)

    def call():
        _ok(lib.st_op_nearest_prepare(vectors, c, m, prepared, _stream()), tag)
        _ok(lib.st_op_nearest_search(feat, c, n, prepared, m, s1, idx, score, _stream()), tag)
        _ok(lib.st_op_nearest_loss(feat, c, n, prepared, m, s2, idx2, unit, loss, _stream()), tag)
        _ok(lib.st_op_nearest_loss_backward(unit, c * n, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('index', range(6))
def test_nearest(index):
    import test_style_nearest_gpu as NN
    n, m = _nearest_shapes()[index]
    c = 64
    # (on the CPU, for these seeds: the gap between the best and the second best float64 distance is at least 8.3e-6 |f_i| max |s_k|
    # on every pixel - above the 5.9e-6 at which tests/test_style_nearest_gpu.py asserts the float64 arg-min)
    f, s = NN._gauss(c, n, 3000 + index), NN._gauss(c, m, 4000 + index)
    _, arg, _ = NN._distances(f, s)
    base = None
    for shift in (SHIFTS if n % 4 == 0 else RAGGED_SHIFTS):
        got = _nearest_run(f, s, shift)
        k = got['idx'].to(torch.int64)
        assert torch.equal(got['idx'], got['idx loss']), (n, m, shift)
        NN._check_deficit(f'caller buffers ({c}, {n}, {m}) shift {shift}', f, s, k)
        assert torch.equal(k, arg), f'({c}, {n}, {m}) shift {shift}: {int((k != arg).sum())} of {n} matches differ from the float64 arg-min'
        want, want_grad = NN._formula(f, s, k)
        ev, eg = _rel(got['loss'][0], want), _gerr(got['grad'], UPSTREAM * want_grad)
        assert ev <= NN.BAR and eg <= NN.BAR, (n, m, shift, ev, eg)
        base = base or got
        assert torch.equal(got['idx'], base['idx'])
        _observe('st_op_nearest_prepare / _search / _loss(_backward)', (c, n, m), shift, got, base)


@pytest.mark.parametrize('offset_bytes', [4, 16, 128])
def test_nearest_refuses_a_misaligned_prepared_or_scratch(offset_bytes):
    lib, (c, n, m) = _lib(), (64, 100, 130)
    g = torch.Generator().manual_seed(6)
    b = Buffers()
    feat, vectors = b.inp('feat', torch.randn((c, n), generator=g)), b.inp('vectors', torch.randn((c, m), generator=g))
    pbytes, sbytes = 4 * int(lib.st_op_nearest_prepared_floats(c, m)), 4 * int(lib.st_op_nearest_scratch_floats(c, n, m))
    good_p, bad_p = b.scratch('prepared', pbytes, 256), b.scratch('prepared off', pbytes, 256, offset_bytes)
    good_s, bad_s = b.scratch('scratch', sbytes, 256), b.scratch('scratch off', sbytes, 256, offset_bytes)
    idx, score, unit, loss = b.out('idx', n, 0, torch.int32), b.out('score', n), b.out('unit', c * n), b.out('loss', 1)
    _ok(lib.st_op_nearest_prepare(vectors, c, m, good_p, _stream()), 'prepare')
    before = b.everything()
    _refused('st_op_nearest_prepare', lib.st_op_nearest_prepare(vectors, c, m, bad_p, _stream()), 'prepared', b, before)
    _refused('st_op_nearest_search', lib.st_op_nearest_search(feat, c, n, bad_p, m, good_s, idx, score, _stream()), 'prepared', b, before)
    _refused('st_op_nearest_search', lib.st_op_nearest_search(feat, c, n, good_p, m, bad_s, idx, score, _stream()), 'scratch', b, before)
    _refused('st_op_nearest_loss', lib.st_op_nearest_loss(feat, c, n, bad_p, m, good_s, idx, unit, loss, _stream()), 'prepared', b, before)
    _refused('st_op_nearest_loss', lib.st_op_nearest_loss(feat, c, n, good_p, m, bad_s, idx, unit, loss, _stream()), 'scratch', b, before)


# =====================================================================================================================
# 6. the sliced Wasserstein entries (csrc/st_sliced.hip: three 1x1 products through launch_conv - csrc/st_conv1x1.hip, fp16x3
#    where conv1x1_split_applies, which asks for 16-byte aligned `in` and weights - the segmented sort, unpack, resample,
#    blend; `scratch` 256-byte aligned)
#    reference and bars: tests/test_style_sliced_gpu.py test_value_gradient_and_determinism - sliced_formula in float64, the
#    value 1e-4, the gradient 1e-4 at the kernels' own stable order (st_op_sliced_project)
# =====================================================================================================================
def _sliced_run(f, style, p, shift):
    lib = _lib()
    (c, n), m = f.shape, style.shape[1]
    si, so = shift
    tag = f'sliced C {c} P {p} n {n} m {m} shift {shift}'
    b = Buffers()
    feat, vectors = b.inp('feat', f, si), b.inp('style', style, si)
    up = b.inp('upstream', torch.tensor([UPSTREAM]), so)
    r, rt = b.out('r', p * c, so), b.out('rt', c * p, so)
    st_, sp, sl = (b.scratch(name, int(lib.st_op_sliced_scratch_bytes(c, p, rows)), 256)
                   for name, rows in (('scratch target', max(n, m)), ('scratch project', n), ('scratch loss', n)))
    target, y = b.out('target', p * n, so), b.out('y', p * n, so)
    unit, loss, grad = b.out('unit', c * n, so), b.out('loss', 1, so), b.out('grad', c * n, so)

    def call():
        _ok(lib.st_op_sliced_directions(11, 0, 0, p, c, r, rt, _stream()), tag)
        _ok(lib.st_op_sliced_target(vectors, c, m, r, rt, p, n, st_, target, 0, 1.0, _stream()), tag)
        _ok(lib.st_op_sliced_project(feat, c, n, r, rt, p, sp, y, _stream()), tag)
        _ok(lib.st_op_sliced_loss(feat, c, n, r, rt, p, target, sl, unit, loss, _stream()), tag)
        _ok(lib.st_op_sliced_loss_backward(unit, c * n, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('c, p', [(64, 64), (128, 64)])
@pytest.mark.parametrize('n, m', [(300, 450), (4097, 3000)])
def test_sliced(c, p, n, m):
    import test_style_sliced_gpu as SG
    from test_style_sliced_cpu import sliced_formula, sliced_target_formula
    f, style = SG._data('relu', c, n, 100 + n), SG._data('relu', c, m, 200 + m)
    base = None
    for shift in (SHIFTS if n % 4 == 0 else RAGGED_SHIFTS):
        got = _sliced_run(f, style, p, shift)
        r64 = got['r'].view(p, c).double().numpy()
        assert torch.equal(got['rt'].view(c, p), got['r'].view(p, c).t().contiguous())
        assert float((got['r'].view(p, c).double().norm(dim=1) - 1).abs().max()) <= 1e-6
        t64 = sliced_target_formula(r64, [style.double().numpy()], [1.0], n)
        want, _ = sliced_formula(f.double().numpy(), r64, t64)
        perm = torch.sort(got['y'].view(p, n) + 0.0, dim=1, stable=True).indices.numpy()
        own_value, own_grad = SG.gradient_at_order(f.double().numpy(), r64, t64, perm)
        rel, err = _rel(got['loss'][0], want), _gerr(got['grad'], UPSTREAM * own_grad)
        assert rel <= SG.BAR and err <= SG.BAR, (c, p, n, m, shift, rel, err)
        assert abs(own_value - want) <= SG.BAR * want
        base = base or got
        assert torch.equal(got['r'], base['r'])                 # the generator does not depend on where its output lies
        _observe('st_op_sliced_directions / _target / _project / _loss(_backward)', (c, p, n, m), shift, got, base)


@pytest.mark.parametrize('offset_bytes', [4, 16, 128])
def test_sliced_refuses_a_misaligned_scratch(offset_bytes):
    lib, (c, p, n) = _lib(), (64, 64, 100)
    g = torch.Generator().manual_seed(7)
    b = Buffers()
    feat = b.inp('feat', torch.randn((c, n), generator=g))
    r = torch.randn((p, c), generator=g)
    pr, prt, ptarget = b.inp('r', r), b.inp('rt', r.t().contiguous()), b.inp('target in', torch.sort(torch.randn((p, n), generator=g), dim=1).values)
    scratch = b.scratch('scratch', int(lib.st_op_sliced_scratch_bytes(c, p, n)), 256, offset_bytes)
    target, y, unit, loss = b.out('target', p * n), b.out('y', p * n), b.out('unit', c * n), b.out('loss', 1)
    before = b.everything()
    _refused('st_op_sliced_target', lib.st_op_sliced_target(feat, c, n, pr, prt, p, n, scratch, target, 0, 1.0, _stream()), 'scratch', b, before)
    _refused('st_op_sliced_project', lib.st_op_sliced_project(feat, c, n, pr, prt, p, scratch, y, _stream()), 'scratch', b, before)
    _refused('st_op_sliced_loss', lib.st_op_sliced_loss(feat, c, n, pr, prt, p, ptarget, scratch, unit, loss, _stream()), 'scratch', b, before)


# =====================================================================================================================
# 7. the Laplacian entries (csrc/st_laplacian.hip launch_lap_pool: VEC = p % 4 == 0, W % 4 == 0 and image aligned;
#    launch_lap_grad: vec = W % 4 == 0 and grad aligned; the residual pass is scalar)
#    reference and bars: tests/test_laplacian_gpu.py test_kernels_alone - the formula in float64, max(2e-6, 3 x the fp32
#    formula's own deviation) for the value, the gradient and the target
# =====================================================================================================================
def _laplacian_run(x, content, pool, shift):
    lib = _lib()
    c, h, w = x.shape
    hp, wp = h // pool, w // pool
    si, so = shift
    tag = f'laplacian {c}x{h}x{w} p {pool} shift {shift}'
    b = Buffers()
    px, pc = b.inp('image', x, si), b.inp('content', content, si)
    up = b.inp('upstream', torch.tensor([1.0]), so)
    nbytes = 4 * int(lib.st_op_laplacian_scratch_floats(c, h, w, pool))
    s1, s2 = b.scratch('scratch target', nbytes, 16, 4 * so), b.scratch('scratch value', nbytes, 16, 4 * so)
    target, residual = b.out('target', c * hp * wp, so), b.out('residual', c * hp * wp, so)
    loss, grad = b.out('loss', 1, so), b.out('grad', c * h * w, so)

    def call():
        _ok(lib.st_op_laplacian_target(pc, c, h, w, pool, s1, target, _stream()), tag)
        _ok(lib.st_op_laplacian_value(px, target, c, h, w, pool, s2, residual, loss, _stream()), tag)
        _ok(lib.st_op_laplacian_backward(residual, c, h, w, pool, up, grad, _stream()), tag)
    call()
    b.verify(tag)
    first = b.bits()
    call()
    b.verify(tag)
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('channels', [1, 3], ids=['C1', 'C3'])
@pytest.mark.parametrize('pool', [1, 2, 4])
@pytest.mark.parametrize('size', [(9, 13), (40, 48)], ids=lambda s: f'{s[0]}x{s[1]}')
def test_laplacian(size, pool, channels):
    import test_laplacian_gpu as LG
    import test_taps_gpu as T
    h, w = size
    x, content = T._smooth(73, h, w)[0, :channels].contiguous(), T._smooth(71, h, w)[0, :channels].contiguous()
    v64, g64, t64, floors, bars = LG._kernel_bars(x, content, pool)
    base = None
    for shift in (SHIFTS if w % 4 == 0 else RAGGED_SHIFTS):
        got = _laplacian_run(x, content, pool, shift)
        grad = got['grad'].view(channels, h, w)
        errs = _rel(got['loss'][0], v64), _gerr(grad, g64), _gerr(got['target'], t64)
        assert all(e <= bar for e, bar in zip(errs, bars)), (size, pool, channels, shift, errs, bars)
        assert torch.count_nonzero(grad[:, h // pool * pool:, :]) == 0 and torch.count_nonzero(grad[:, :, w // pool * pool:]) == 0
        base = base or got
        _observe('st_op_laplacian_target / _value / _backward', (channels, h, w, pool), shift, got, base)


# =====================================================================================================================
# 8. L-BFGS (csrc/st_lbfgs.hip launch_lbfgs_update: vec = count % 4 == 0 and state, image, grad, ema 16-byte aligned; the state
#    must be 16-byte aligned)
#    reference and bars: tests/test_lbfgs_gpu.py - torch.optim.LBFGS on the CPU fed the same gradients; a constant gradient:
#    every iterate within 4 ulp of the largest; a zero gradient: nothing moves, the EMA within 1 ulp
# =====================================================================================================================
def _lbfgs_run(x0, grads, shift):
    lib, count = _lib(), x0.numel()
    si, so = shift
    tag = f'lbfgs count {count} shift {shift}'
    b = Buffers()
    state = b.scratch('state', int(lib.st_lbfgs_state_bytes(count)), 16)
    image, ema = b.inout('image', x0, so), b.inout('ema', torch.zeros_like(x0), so)
    gptrs = [b.inp(f'grad {k}', g, si) for k, g in enumerate(grads)]
    runs = []
    for _ in range(2):            # the second sequence starts from the state the first left: st_lbfgs_reset makes it fresh
        b.items['image'][1].copy_(x0.flatten())
        b.items['ema'][1].zero_()
        _ok(lib.st_lbfgs_reset(state, count, _stream()), tag)
        iterates = []
        for gp in gptrs:
            _ok(lib.st_lbfgs_update(state, count, image, gp, ema, 0.99, _stream()), tag)
            b.verify(tag)
            iterates.append(b.get('image').view(x0.shape))
        assert torch.isfinite(b.get('ema')).all() and torch.isfinite(iterates[-1]).all(), tag
        runs.append((iterates, b.get('ema').view(x0.shape)))
    for a, c in zip(runs[0][0], runs[1][0]):
        assert torch.equal(a, c), f'{tag}: a second sequence after st_lbfgs_reset gave other bits'
    assert torch.equal(runs[0][1], runs[1][1]), tag
    return runs[0]


@pytest.mark.parametrize('shape', [(3, 40, 48), (3, 45, 54)], ids=lambda s: 'x'.join(map(str, s)))
def test_lbfgs_update(shape):
    import test_lbfgs_gpu as LB
    gen = torch.Generator().manual_seed(4)
    x0 = torch.rand(shape, generator=gen)
    g = torch.rand(shape, generator=gen) - 0.3
    want, _ = LB._torch_lbfgs_on(x0, [g] * 3)
    count = x0.numel()
    shifts = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 3), (3, 2)] if count % 4 == 0 else RAGGED_SHIFTS
    base = None
    for shift in shifts:
        got, _ = _lbfgs_run(x0, [g] * 3, shift)
        for k in range(3):
            bound = 4 * ULP * float(want[k].abs().max())
            assert float((got[k] - want[k]).abs().max()) <= bound, (shape, shift, k)
        still, value = _lbfgs_run(x0, [torch.zeros(shape)] * 2, shift)
        assert torch.equal(still[-1], x0)
        e, d = torch.zeros(shape), torch.tensor(0.99)
        for _ in range(2):
            e = e * d + (1 - d) * x0
        assert float((value - e).abs().max()) <= ULP, (shape, shift)
        base = base or {'image': got[-1]}
        _observe('st_lbfgs_reset / _update', shape, shift, {'image': got[-1]}, base)


@pytest.mark.parametrize('offset_bytes', [4, 8])
def test_lbfgs_refuses_a_misaligned_state(offset_bytes):
    lib, count = _lib(), 3 * 16 * 16
    b = Buffers()
    state = b.scratch('state', int(lib.st_lbfgs_state_bytes(count)), 16, offset_bytes)
    image, ema = b.inout('image', torch.rand(count)), b.inout('ema', torch.zeros(count))
    grad = b.inp('grad', torch.rand(count))
    before = b.everything()
    _refused('st_lbfgs_reset', lib.st_lbfgs_reset(state, count, _stream()), 'state', b, before)
    _refused('st_lbfgs_update', lib.st_lbfgs_update(state, count, image, grad, ema, 0.99, _stream()), 'state', b, before)


def test_plan_lbfgs_step_refuses_a_misaligned_state():
    import test_taps_gpu as T
    lib, size = _lib(), (40, 48)
    net, plan = _default_plan(size, 'fp16x3')
    n = 3 * size[0] * size[1]
    for offset_bytes in (4, 8):
        b = Buffers()
        state = b.scratch('state', int(lib.st_lbfgs_state_bytes(n)), 16, offset_bytes)
        x, ema = b.inout('x', T._inputs(size, 'max')['image'].flatten()), b.inout('ema', torch.zeros(n))
        losses = b.out('losses', 8)
        before = b.everything()
        _refused('st_plan_lbfgs_step', lib.st_plan_lbfgs_step(plan.handle, x, state, ema, 0.99, losses, _stream()), 'state', b, before)


# =====================================================================================================================
# 9. the 1x1 step (csrc/st_conv.hip launch_conv: with the scratch st_op_conv1x1 hands it, a problem of fewer than 512 256-pixel
#    tiles splits K while 2 x (128-pixel workgroups) <= 640; only with ksplit == 1 does precision 4 reach launch_conv1x1_split,
#    the fp16x3 tile kernel, and then only when `in` and the weights are 16-byte aligned - csrc/st_conv1x1.hip:185; everything
#    else is the generic kernel on the fp32 MFMA.  (128, 37), (512, 4096) [256 workgroups] and (64, 40001) [313] split K in both
#    precisions; (64, 208 x 208) [338] and (64, 208 x 208 + 1) [339, ragged tiles] keep ksplit == 1: fp16x3 tiles when aligned)
#    reference and bars: tests/test_kernels_gpu.py test_conv1x1_head_gradient_step - float64, rel-L2 1e-6 (fp32) / 2e-6 (fp16x3)
# =====================================================================================================================
CONV1X1_SHAPES = [(128, 37), (512, 4096), (64, 40001), (64, 208 * 208), (64, 208 * 208 + 1)]
CONV1X1_F16 = [(64, 208 * 208), (64, 208 * 208 + 1)]          # ksplit == 1: precision 4 is conv1x1_f16_kernel


def _conv1x1_run(x, s, bias, precision, shift):
    lib = _lib()
    c, npix = x.shape
    si, so = shift
    tag = f'conv1x1 C {c} npix {npix} precision {precision} shift {shift}'
    b = Buffers()
    pin, pw, pb = b.inp('in', x, si), b.inp('weight', s, si), b.inp('bias', bias, si)
    out = b.out('out', c * npix, so)
    for k in range(2):
        _ok(lib.st_op_conv1x1(pin, pw, pb, out, c, c, npix, precision, _stream()), tag)
        b.verify(tag)
        first = b.bits() if k == 0 else first
    _same_bits(tag, first, b.bits())
    return {'out': b.get('out')}


@pytest.mark.parametrize('precision', [0, 4])
@pytest.mark.parametrize('c, npix', CONV1X1_SHAPES)
def test_conv1x1(c, npix, precision):
    g = torch.Generator().manual_seed(c + npix)
    x = torch.relu(torch.randn((c, npix), generator=g)) * torch.exp(2 * torch.randn((c, 1), generator=g))
    s = torch.randn((c, c), generator=g) * torch.exp(3 * torch.randn((c, c), generator=g)) * 1e-7
    s = s + s.t()
    bias = torch.randn((c,), generator=g) * 1e-6
    want = (s.double() @ x.double() + bias.double()[:, None]).float()
    base = None
    for shift in (SHIFTS if npix % 4 == 0 else RAGGED_SHIFTS + [(3, 1)]):
        got = _conv1x1_run(x, s, bias, precision, shift)
        err = rel_l2(got['out'].view(c, npix), want)
        assert np.isfinite(err) and err <= (2e-6 if precision else 1e-6), (c, npix, precision, shift, err)
        base = base or got
        _observe(f'st_op_conv1x1 precision {precision}', (c, npix), shift, got, base)
        if precision == 4 and (c, npix) in CONV1X1_F16:
            # which kernel ran, from the bits: with `in` and the weights aligned the result differs from the precision-0 result
            # (fp16x3 planes and the fp32 MFMA cannot agree in bits) and does not depend on where `out` lies; with them
            # shifted another kernel runs, so the bits differ from the aligned run's (the split-K shapes above give equal bits
            # at every shift: there one kernel serves all of them)
            if shift[0] == 0:
                assert not torch.equal(got['out'], _conv1x1_run(x, s, bias, 0, shift)['out']), (c, npix, shift)
                assert torch.equal(got['out'], base['out']), (c, npix, shift)
            else:
                assert not torch.equal(got['out'], base['out']), (c, npix, shift)


# =====================================================================================================================
# 10. the 3x3 convolution (csrc/st_conv.hip, st_conv_split.hip, st_conv_pc.hip, st_conv_fat.hip: the epilogue's 16-byte path
#     when W % 4 == 0 and out / out_mask are aligned; the halo rows of a strip)
#     reference and bars: tests/test_kernels_gpu.py test_conv3x3_forward / _data_gradient_with_relu_mask - torch's fp32 CPU
#     convolution, rel-L2 2e-6 (precision 0) / 3e-6 (precision 4)
# =====================================================================================================================
CONV_CASES = [(64, 64, 40, 48), (128, 128, 9, 100), (256, 512, 5, 5), (64, 64, 9, 13)]
CONV_TOL = {0: 2e-6, 4: 3e-6}


def _conv_operands(cin, cout, h, w):
    g = torch.Generator().manual_seed(cin * 7 + cout + h * 3 + w)
    x = torch.randn((1, cin, h + 2, w), generator=g)              # rows 1 .. h are the tensor (or the strip); 0 and h + 1 its halo
    wt = torch.randn((cout, cin, 3, 3), generator=g) * (2.0 / (cin * 9)) ** 0.5
    bias = torch.randn((cout,), generator=g) * 0.1
    gy = torch.randn((1, cout, h, w), generator=g)
    mask = torch.randn((cout, h, w), generator=g)
    return x, wt, bias, gy, mask


def _conv_run(cin, cout, h, w, precision, shift):
    lib = _lib()
    si, so = shift
    tag = f'conv3x3 {cin}->{cout} {h}x{w} precision {precision} shift {shift}'
    x, wt, bias, gy, mask = _conv_operands(cin, cout, h, w)
    inner = x[:, :, 1:h + 1].contiguous()
    y = TF.conv2d(inner, wt, bias, padding=1).relu()
    b = Buffers()
    pin, pw, pb = b.inp('in', inner, si), b.inp('weight', wt, si), b.inp('bias', bias, si)
    pgy, py = b.inp('grad_out', gy, si), b.inp('relu_out', y, si)
    halo = b.inp('halo', torch.stack([x[0, :, 0], x[0, :, h + 1]]), si)
    pmask = b.inp('out_mask', mask, so)
    out, grad_in, strip = b.out('out', cout * h * w, so), b.out('grad_in', cin * h * w, so), b.out('strip', cout * h * w, so)
    for k in range(2):
        _ok(lib.st_op_conv3x3(pin, pw, pb, out, cin, cout, h, w, 1, precision, _stream()), tag)
        _ok(lib.st_op_conv3x3_dgrad(pgy, py, pw, grad_in, cin, cout, h, w, precision, _stream()), tag)
        _ok(lib.st_op_conv3x3_strip_ex(pin, halo, 1, 1, pw, pb, strip, pmask, cin, cout, h, w, 1, 0, 0, 0, precision, _stream()), tag)
        b.verify(tag)
        first = b.bits() if k == 0 else first
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('precision', [0, 4])
@pytest.mark.parametrize('cin, cout, h, w', CONV_CASES)
def test_conv3x3(cin, cout, h, w, precision):
    x, wt, bias, gy, mask = _conv_operands(cin, cout, h, w)
    inner = x[:, :, 1:h + 1].clone().requires_grad_(True)
    y = TF.conv2d(inner, wt, bias, padding=1).relu()
    y.backward(gy)
    tall = TF.conv2d(x, wt, bias, padding=1)[0, :, 1:h + 1].relu()
    want_strip = torch.where(mask > 0, tall, torch.zeros(()))
    tol = CONV_TOL[precision]
    base = None
    for shift in (SHIFTS if w % 4 == 0 else RAGGED_SHIFTS):
        got = _conv_run(cin, cout, h, w, precision, shift)
        errs = (rel_l2(got['out'].view(y.shape), y.detach()), rel_l2(got['grad_in'].view(inner.shape), inner.grad),
                rel_l2(got['strip'].view(tall.shape), want_strip))
        assert all(np.isfinite(e) and e <= tol for e in errs), (cin, cout, h, w, precision, shift, errs)
        assert bool((got['strip'].view(tall.shape)[mask <= 0] == 0).all())
        base = base or got
        _observe(f'st_op_conv3x3 / _dgrad / _strip_ex precision {precision}', (cin, cout, h, w), shift, got, base)


# =====================================================================================================================
# 11. the Newton-Schulz square root (csrc/st_nschain.hip, st_nsgemm.hip: no branch on the caller's pointers)
#     reference and bars: tests/test_kernels_gpu.py test_sqrtm_against_oracle - the oracle's 12 iterations, rel-L2 2e-5 forward,
#     2e-4 backward
# =====================================================================================================================
def _sqrtm_run(a, root, gout, gdiag, shift):
    lib, n = _lib(), a.shape[0]
    si, so = shift
    tag = f'sqrtm n {n} shift {shift}'
    b = Buffers()
    pa, proot, pg = b.inp('a', a, si), b.inp('root in', root, si), b.inp('grad_root', gout, si)
    out, ga, gd = b.out('root', n * n, so), b.out('grad_a', n * n, so), b.out('grad_a diag', n * n, so)
    for k in range(2):
        _ok(lib.st_op_sqrtm_ns(pa, out, n, _stream()), tag)
        _ok(lib.st_op_sqrtm_ns_backward(proot, pg, ga, n, _stream()), tag)
        _ok(lib.st_op_sqrtm_ns_backward_diag(proot, gdiag, gd, n, _stream()), tag)
        b.verify(tag)
        first = b.bits() if k == 0 else first
    _same_bits(tag, first, b.bits())
    return {name: b.get(name) for name in first}


@pytest.mark.parametrize('n', [64, 128])
def test_sqrtm(n):
    g = torch.Generator().manual_seed(n)
    m = torch.randn((n, 2 * n), generator=g)
    a = (m @ m.t()) / (2 * n) + torch.eye(n) * 1e-2
    want = O.ns_sqrt(a, 12)
    gout = torch.randn((n, n), generator=g)
    want_b = O.ns_sqrt_bwd(want, gout, 12)
    gdiag = -2.0 / n
    want_d = O.ns_sqrt_bwd(want, gdiag * torch.eye(n), 12)
    base = None
    for shift in SHIFTS:
        got = _sqrtm_run(a, want, gout, gdiag, shift)
        errs = rel_l2(got['root'].view(n, n), want), rel_l2(got['grad_a'].view(n, n), want_b), rel_l2(got['grad_a diag'].view(n, n), want_d)
        assert errs[0] <= 2e-5 and errs[1] <= 2e-4 and errs[2] <= 2e-4, (n, shift, errs)
        base = base or got
        _observe('st_op_sqrtm_ns / _backward / _backward_diag', n, shift, got, base)


# =====================================================================================================================
# 12. the standalone style head (csrc/st_head.hip: feat, state and grad_feat must be 16-byte aligned - the Gram kernels and the
#     1x1 step stage them in 16-byte groups without a scalar sibling; mean_out, srm_out and loss_out need not be)
#     reference and bars: tests/test_native_losses_gpu.py - Scale(module.double(), 0.37) on the CPU, value and gradient 1e-4,
#     moments 1e-6 against float64 moments of the same input
# =====================================================================================================================
HEAD_SHAPES = [(64, 9, 13), (512, 5, 6)]
HEAD_BIG = (64, 208, 208)          # the smallest shape on which the backward's 1x1 step is the fp16x3 kernel


def _head_run(kind, shape, module, x, out_shift, precision=4):
    lib = _lib()
    c, h, w = shape
    tag = f'head {kind} {shape} targets and outputs shifted {out_shift}'
    handle = ctypes.c_void_p()
    _ok(lib.st_head_create(ctypes.byref(handle), 0 if kind == 'w2' else 1, c, h, w, precision), tag)
    try:
        n_state = int(lib.st_head_state_floats(handle))
        b = Buffers()
        feat = b.inp('feat', x[0])
        up = b.inp('upstream', torch.tensor([UPSTREAM]), out_shift)
        if kind == 'w2':
            targets = [b.inp(name, t, out_shift) for name, t in (('mean_t', module.mean), ('cov_t', module.cov), ('root_t', module.cov_sqrt))] + [None]
            eps = float(module.eps)
        else:
            targets = [None, None, None, b.inp('gram_t', module.target, out_shift)]
            eps = float(module.loss.eps)
        mean, srm = b.out('mean', c, out_shift), b.out('srm', c * c, out_shift)
        loss, state, grad = b.out('loss', 1, out_shift), b.opaque('state', n_state), b.out('grad_feat', c * h * w)

        def call():
            _ok(lib.st_head_moments(handle, feat, mean, srm, _stream()), tag)
            _ok(lib.st_head_forward(handle, feat, *targets, eps, loss, state, _stream()), tag)
            _ok(lib.st_head_backward(handle, feat, state, up, grad, _stream()), tag)
        def bits():          # of the state, (Ssym, b): the bound behind them is a set of atomicMax slots, of which the largest is read
            out = b.bits()
            out['state'] = out['state'][:c * c + c]
            return out
        call()
        b.verify(tag)
        first = bits()
        call()
        b.verify(tag)
        _same_bits(tag, first, bits())
        got = {name: b.get(name) for name in first}
        got['state'] = got['state'][:c * c + c]
        # offsets 1 to 3 on feat / state / grad_feat: the documented refusal, and nothing is written
        if out_shift == 0:
            before = b.everything()
            for k in (1, 2, 3):
                f_off, s_off, g_off = (ctypes.c_void_p(b.ptr(name).value + 4 * k) for name in ('feat', 'state', 'grad_feat'))
                _refused(f'st_head_moments feat + {k}', lib.st_head_moments(handle, f_off, mean, srm, _stream()), 'feat', b, before)
                _refused(f'st_head_forward feat + {k}', lib.st_head_forward(handle, f_off, *targets, eps, loss, state, _stream()), 'feat', b, before)
                _refused(f'st_head_forward state + {k}', lib.st_head_forward(handle, feat, *targets, eps, loss, s_off, _stream()), 'state', b, before)
                _refused(f'st_head_backward feat + {k}', lib.st_head_backward(handle, f_off, state, up, grad, _stream()), 'feat', b, before)
                _refused(f'st_head_backward state + {k}', lib.st_head_backward(handle, feat, s_off, up, grad, _stream()), 'state', b, before)
                _refused(f'st_head_backward grad_feat + {k}', lib.st_head_backward(handle, feat, state, up, g_off, _stream()), 'grad_feat', b, before)
        return got
    finally:
        _sync()
        lib.st_head_destroy(handle)


def _head_check(kind, shape, out_shifts):
    import test_native_losses_gpu as NL
    module, x, v64, g64 = NL._case(kind, shape, True)
    c = shape[0]
    f64 = x[0].double().flatten(1)
    want_mean, want_srm = f64.mean(1), (f64 @ f64.t()) / f64.shape[1]
    base = None
    for out_shift in out_shifts:
        got = _head_run(kind, shape, module, x, out_shift)
        ev, eg = _rel(UPSTREAM * float(got['loss'][0]), v64), _gerr(got['grad_feat'], g64)
        assert ev <= NL.value_bar(kind) and eg <= NL.grad_bar(kind), (kind, shape, out_shift, ev, eg)
        assert rel_l2(got['mean'], want_mean) <= NL.MOMENT_TOL and rel_l2(got['srm'].view(c, c), want_srm) <= NL.MOMENT_TOL
        assert torch.equal(got['srm'].view(c, c), got['srm'].view(c, c).t()), 'srm_out is exactly symmetric'
        base = base or got
        _observe(f'st_head_moments / _forward / _backward ({kind})', shape, out_shift, got, base)


@pytest.mark.parametrize('shape', HEAD_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('kind', ['w2', 'gram'])
def test_head(kind, shape):
    _head_check(kind, shape, (0, 1, 2, 3))


def test_head_on_the_fp16x3_1x1_kernel():
    _head_check('w2', HEAD_BIG, (0, 3))


# =====================================================================================================================
# 13. the plan entries: caller-owned image, gradient, losses, Adam moments, EMA, L-BFGS state, tap moments - and the setters
#     that read caller memory.  One Net per precision, plans at 40 x 48 (W % 4 == 0) and 45 x 54 (not).
#     reference and bars: tests/test_taps_gpu.py _judge - the oracle in float32 and float64 on the plan's own ReLU / pool
#     decisions: a term max(1e-4, 3 x its fp32 floor), the total 1e-6 of the fp32 sum, the gradient bar(floor)
# =====================================================================================================================
PLAN_SIZES = [(40, 48), (45, 54)]
PLAN_SHIFTS = [dict(image=0, grad=0, moments=0, ema=0), dict(image=1, grad=2, moments=3, ema=1)]
ADAM = (0.02, 0.9, 0.99, 1e-8, 0.99)


def _default_plan(size, precision, graph=False):
    import test_taps_gpu as T
    net, plan = T._configured_plan(size, 'max', precision, *T.DEFAULT, configure=False)
    if graph:
        plan.set_graph(True)
    return net, plan


def _closure_buffers(image, shift):
    b = Buffers()
    n = image.numel()
    ptrs = b.inp('image', image, shift['image']), b.out('grad', n, shift['grad']), b.out('losses', 8, shift['grad'])
    return b, ptrs


def _run_closure(plan, b, ptrs, tag):
    _ok(_lib().st_plan_loss_and_grad(plan.handle, *ptrs, _stream()), tag)
    b.verify(tag)
    return b.bits()


@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('precision', ['fp16x3', 'fp32'])
def test_plan_closure_against_the_oracle(precision, size):
    import test_taps_gpu as T
    image = T._inputs(size, 'max')['image']
    img = image.to(DEV)
    net, plan = _default_plan(size, precision)
    base = None
    for shift in PLAN_SHIFTS:
        tag = f'{size[0]}x{size[1]}-{precision} default closure, shift {shift}'
        b, ptrs = _closure_buffers(image, shift)

        def closure():
            first = _run_closure(plan, b, ptrs, tag)
            _same_bits(tag, first, _run_closure(plan, b, ptrs, tag))
            return b.items['losses'][1], b.items['grad'][1].view(1, 3, *size)
        _, _, _, failures = T._judge(tag, plan, img, image, 'max', *T.DEFAULT, closure)
        assert not failures, '; '.join(failures)
        got = {'grad': b.get('grad'), 'losses': b.get('losses')}
        base = base or got
        _observe(f'st_plan_loss_and_grad ({precision})', size, shift, got, base)


def _maps(size):
    h, w = size
    g = torch.Generator().manual_seed(h * 100 + w)
    ramp = torch.linspace(0.2, 1.0, w)[None, :].expand(h, w)
    return dict(style=(0.25 + 0.75 * torch.rand((h, w), generator=g)).contiguous(), content=ramp.contiguous(),
                tv=(0.5 + 0.5 * torch.rand((h, w), generator=g)).contiguous())


def _set_maps(plan, size, shift):
    import test_taps_gpu as T
    lib = _lib()
    maps = _maps(size)
    b = Buffers()
    tag = f'setters {size} shift {shift}'
    _ok(lib.st_plan_set_style_mask(plan.handle, b.inp('style mask', maps['style'], shift), _stream()), tag)
    _ok(lib.st_plan_set_content_mask(plan.handle, b.inp('content map', maps['content'], shift), _stream()), tag)
    _ok(lib.st_plan_set_tv_mask(plan.handle, b.inp('tv map', maps['tv'], shift), _stream()), tag)
    pools = (ctypes.c_int * 2)(1, 4)
    _ok(lib.st_plan_set_laplacian(plan.handle, b.inp('laplacian content', T._smooth(71, *size)[0], shift), 2, pools, 10.0, _stream()), tag)
    ctargets, moments = T._targets(size, 'max', *T.DEFAULT)
    _ok(lib.st_plan_set_content_target(plan.handle, b.inp('content target', ctargets[22], shift), _stream()), tag)
    for i, layer in enumerate(T.DEFAULT[1]):
        _ok(lib.st_plan_set_style_target(plan.handle, i, b.inp(f'mean {layer}', moments[layer][0], shift),
                                         b.inp(f'srm {layer}', moments[layer][1], shift), _stream()), tag)
    b.verify(tag)
    return b


@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plan_setters_and_the_general_closure(size):
    """The setters that read caller memory, fed from fenced buffers at offset 0 and off alignment: what the plan then
    computes - the general closure with a style mask, a content map, a TV map and a Laplacian - must be the same bits, on
    caller buffers that are themselves aligned and shifted."""
    import test_taps_gpu as T
    image = T._inputs(size, 'max')['image']
    results = {}
    for setter_shift in (0, 1, 2, 3):
        net, plan = _default_plan(size, 'fp16x3')
        keep = _set_maps(plan, size, setter_shift)
        for shift in (PLAN_SHIFTS if setter_shift in (0, 2) else PLAN_SHIFTS[:1]):
            tag = f'{size[0]}x{size[1]} general closure, setters at {setter_shift}, shift {shift}'
            b, ptrs = _closure_buffers(image, shift)
            first = _run_closure(plan, b, ptrs, tag)
            _same_bits(tag, first, _run_closure(plan, b, ptrs, tag))
            results[(setter_shift, shift['image'])] = {'grad': b.get('grad'), 'losses': b.get('losses')}
        keep.verify(f'setters {size}')
        del plan, net
    base = results[(0, 0)]
    for (setter_shift, image_shift), got in results.items():
        if image_shift == 0:
            assert torch.equal(got['grad'], base['grad']) and torch.equal(got['losses'], base['losses']), \
                f'{size}: setters fed from buffers {setter_shift} floats off alignment give another plan'
        _observe('st_plan_set_* + general closure', size, (setter_shift, image_shift), got, base)
    # (the closure itself is held to the oracle at both offsets by test_plan_general_closure_against_the_oracle)
    assert torch.equal(results[(0, 1)]['grad'], results[(2, 1)]['grad'])


def _step_buffers(image, shift):
    b = Buffers()
    x = image.flatten()
    ptrs = (b.inout('image', x, shift['image']), b.inout('exp_avg', torch.zeros_like(x), shift['moments']),
            b.inout('exp_avg_sq', torch.zeros_like(x), shift['moments']), b.inout('ema', 0.01 * x, shift['ema']))
    return b, ptrs, b.out('losses', 8, shift['grad'])


@pytest.mark.parametrize('graph', [False, True], ids=['eager', 'graph'])
@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plan_step_and_apply_update(size, graph):
    """st_plan_step on fenced, shifted state - eager (the update rides in conv1_1's fold kernel, ST_STEP_TAIL 2) and under graph
    replay (launch of its own) - is st_plan_loss_and_grad followed by st_plan_apply_update on the same buffers, bit for bit
    (tests/test_taps_gpu.py test_step_is_loss_and_grad_plus_update_bit_for_bit).  The two halves have their references: the
    closure the oracle (test_plan_closure_against_the_oracle), the update float64 (test_plan_apply_update_against_float64)."""
    import test_taps_gpu as T
    lib = _lib()
    image = T._inputs(size, 'max')['image']
    lr, b1, b2, eps, decay = ADAM
    results = []
    for shift in PLAN_SHIFTS:
        tag = f'{size[0]}x{size[1]} step graph={graph} shift {shift}'
        net, plan = _default_plan(size, 'fp16x3', graph)
        b, ptrs, losses = _step_buffers(image, shift)
        for k in (1, 2, 3):
            _ok(lib.st_plan_step(plan.handle, *ptrs, k, lr, b1, b2, eps, decay, losses, _stream()), tag)
            b.verify(tag)
        stepped = b.bits()
        assert all(bool(torch.isfinite(b.get(name)).all()) for name in stepped), tag
        # the same three iterations as closure + update, on buffers of the same shifts
        net2, plan2 = _default_plan(size, 'fp16x3', graph)
        b2_, ptrs2, _ = _step_buffers(image, shift)
        grad, losses2 = b2_.out('grad', image.numel(), shift['grad']), b2_.out('losses', 8, shift['grad'])
        for k in (1, 2, 3):
            _ok(lib.st_plan_loss_and_grad(plan2.handle, ptrs2[0], grad, losses2, _stream()), tag)
            _ok(lib.st_plan_apply_update(plan2.handle, ptrs2[0], grad, *ptrs2[1:], k, lr, b1, b2, eps, decay, _stream()), tag)
            b2_.verify(tag)
        split = b2_.bits()
        for name in ('image', 'exp_avg', 'exp_avg_sq', 'ema', 'losses'):
            assert torch.equal(stepped[name], split[name]), f'{tag}: {name}: step differs from closure + update'
        results.append({name: b.get(name) for name in stepped})
    _observe(f'st_plan_step graph={graph}', size, PLAN_SHIFTS[1], results[1], results[0])


@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plan_apply_update_against_float64(size):
    """st_plan_apply_update (csrc/st_pointwise.hip launch_adam_clamp_ema) on fenced image, gradient, moments and EMA, aligned and
    shifted.  Reference and bar: tests/test_update_gpu.py - ref_update64, the update in float64, on chosen_state (gradients over
    six decades, exact zeros, pixels at both clamps); each tensor within 4 x the floor of torch.optim.Adam in fp32."""
    import test_update_gpu as UP
    lib = _lib()
    net, plan = _default_plan(size, 'fp16x3')
    state = UP.chosen_state(*size)
    g, m, v, p, e = state
    for shift in PLAN_SHIFTS:
        for step in (1, 10):
            tag = f'{size[0]}x{size[1]} apply_update step {step} shift {shift}'
            b = Buffers()
            ptrs = (b.inout('image', p, shift['image']), b.inp('grad', g, shift['grad']), b.inout('exp_avg', m, shift['moments']),
                    b.inout('exp_avg_sq', v, shift['moments']), b.inout('ema', e, shift['ema']))
            _ok(lib.st_plan_apply_update(plan.handle, *ptrs, step, *UP.SHIPPED, _stream()), tag)
            b.verify(tag)
            got = tuple(b.get(name).view(g.shape) for name in ('exp_avg', 'exp_avg_sq', 'image', 'ema'))
            failures = UP.judge(tag, got, state, step, UP.SHIPPED)
            assert not failures, '; '.join(failures)


def test_plan_pointer_change_under_graph_replay():
    """The captured graph is keyed on (image, grad_out, losses_out): buffers A, then B (another address, another offset),
    then A again on one graph-enabled plan.  Each result equals, in bits, what a fresh plan gives for that buffer, and the
    buffer that is not the call's is not touched."""
    import test_taps_gpu as T
    size = (40, 48)
    image_a, image_b = T._inputs(size, 'max')['image'], T._smooth(91, *size)
    fresh = {}
    for name, image, shift in (('A', image_a, PLAN_SHIFTS[0]), ('B', image_b, PLAN_SHIFTS[1])):
        net, plan = _default_plan(size, 'fp16x3')
        b, ptrs = _closure_buffers(image, shift)
        fresh[name] = _run_closure(plan, b, ptrs, f'fresh plan, buffers {name}')
        del plan, net
    net, plan = _default_plan(size, 'fp16x3', graph=True)
    (ba, pa), (bb, pb) = _closure_buffers(image_a, PLAN_SHIFTS[0]), _closure_buffers(image_b, PLAN_SHIFTS[1])
    for name in ('A', 'A', 'B', 'B', 'A', 'B', 'A'):
        mine, ptrs, other = (ba, pa, bb) if name == 'A' else (bb, pb, ba)
        before = other.everything()
        got = _run_closure(plan, mine, ptrs, f'graph plan, buffers {name}')
        after = other.everything()
        assert all(torch.equal(before[k], after[k]) for k in before), f'buffers {name}: the other call\'s buffers were written'
        _same_bits(f'graph plan, buffers {name} against a fresh plan', fresh[name], got)
        for _, view, whole in (mine.items['grad'], mine.items['losses']):          # poison the outputs again: a replay must rewrite them
            F._ints(view).fill_(F.POISON)


@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
@pytest.mark.parametrize('precision', ['fp16x3', 'fp32'])
def test_plan_general_closure_against_the_oracle(precision, size):
    """The general closure with a style mask, a content map, a TV map and a Laplacian (pools 1 and 4) - every image-space kernel -
    on fenced buffers at both PLAN_SHIFTS, held to the oracle as tests/test_laplacian_gpu.py holds
    test_closure_with_a_style_mask_a_content_map_and_a_tv_map: every term max(1e-4, 3 x its fp32 floor), the gradient bar(floor)."""
    import test_laplacian_gpu as LG
    import test_taps_gpu as T
    from test_style_mask_gpu import binary_mask, ramp_mask
    image = T._inputs(size, 'max')['image']
    img = image.to(DEV)
    net, plan = _default_plan(size, precision)
    plan.set_content_mask(ramp_mask(*size).to(DEV))
    plan.set_tv_mask(binary_mask(*size).to(DEV))
    plan.set_style_mask(ramp_mask(size[1], size[0]).t().contiguous().to(DEV))
    base = None
    for shift in PLAN_SHIFTS:
        tag = f'{size[0]}x{size[1]}-{precision} general closure with three maps and a Laplacian, shift {shift}'
        plan.set_laplacian(None)                       # the judge sets it itself, after a closure without
        b, ptrs = _closure_buffers(image, shift)

        def closure():
            first = _run_closure(plan, b, ptrs, tag)
            _same_bits(tag, first, _run_closure(plan, b, ptrs, tag))
            return b.items['losses'][1], b.items['grad'][1].view(1, 3, *size)
        failures = LG._judge(tag, plan, img, image, size, 'max', *T.DEFAULT, ('mse', 'w2'), (1, 4), closure=closure)
        assert not failures, '; '.join(failures)
        got = {'grad': b.get('grad'), 'losses': b.get('losses')}
        base = base or got
        _observe(f'general closure, three maps and a Laplacian ({precision})', size, shift, got, base)


@pytest.mark.parametrize('size', PLAN_SIZES, ids=lambda s: f'{s[0]}x{s[1]}')
def test_plan_forward_moments_backward_and_lbfgs_step(size):
    """st_plan_forward (image), st_plan_moments (mean_out, srm_out), st_plan_backward (grads, grad_image) and
    st_plan_lbfgs_step (image, state, ema_value, losses_out) on fenced buffers, aligned and shifted.
    References and bars: the taps and moments do not depend on where the caller's buffers lie (equal bits) and the moments are
    within 1e-6 of float64 moments of the plan's own tap (tests/test_kernels_gpu.py test_moments_of_taps); grad_image against the
    oracle's vector-Jacobian product in float64 on the plan's branches at bar(fp32 floor) (tests/test_vgg_backward_gpu.py);
    st_plan_lbfgs_step is st_plan_loss_and_grad + st_lbfgs_update on buffers of the same offsets, bit for bit
    (tests/test_taps_gpu.py test_lbfgs_step_is_loss_and_grad_plus_update_bit_for_bit) - the closure is held to the oracle and
    the update to torch.optim.LBFGS above."""
    import test_taps_gpu as T
    import test_vgg_backward_gpu as VB
    lib = _lib()
    image = T._inputs(size, 'max')['image']
    n = image.numel()
    taps = (1, 6, 29)
    runs = []
    for shift in PLAN_SHIFTS:
        tag = f'{size[0]}x{size[1]} forward / moments / backward / lbfgs shift {shift}'
        net, plan = _default_plan(size, 'fp16x3')
        b = Buffers()
        pimg = b.inp('image', image, shift['image'])
        _ok(lib.st_plan_forward(plan.handle, pimg, 29, _stream()), tag)
        feats = {layer: plan.feature(layer).clone() for layer in taps}
        decisions = VB._decisions(plan, 'max')
        for layer in (1, 29):
            c = feats[layer].shape[-3]
            _ok(lib.st_plan_moments(plan.handle, layer, b.out(f'mean {layer}', c, shift['moments']),
                                    b.out(f'srm {layer}', c * c, shift['moments']), _stream()), tag)
        cots = {layer: VB._cot(layer, feats[layer].shape) for layer in taps}
        layers = (ctypes.c_int * 3)(*taps)
        gptrs = (ctypes.c_void_p * 3)(*[b.inp(f'cotangent {layer}', cots[layer], shift['grad']).value for layer in taps])
        _ok(lib.st_plan_backward(plan.handle, 3, layers, gptrs, b.out('grad_image', n, shift['grad']), _stream()), tag)
        b.verify(tag)
        (g32,), (g64,) = (VB._oracle_vjps(image, 'max', decisions, cots, [taps], dtype) for dtype in (torch.float32, torch.float64))
        failures = []
        VB._judge(tag, b.get('grad_image').view(1, 3, *size), g64, g32, failures)
        assert not failures, '; '.join(failures)
        # the L-BFGS step, three iterations on fenced state, and the same as closure + update on buffers of the same offsets
        pairs = []
        for name in ('step', 'split'):
            state = b.scratch(f'lbfgs state {name}', int(lib.st_lbfgs_state_bytes(n)), 16)
            x, ema = b.inout(f'x {name}', image.flatten(), shift['image']), b.inout(f'ema {name}', torch.zeros(n), shift['ema'])
            losses = b.out(f'losses {name}', 8, shift['grad'])
            grad = b.out('grad split', n, shift['grad']) if name == 'split' else None
            _ok(lib.st_lbfgs_reset(state, n, _stream()), tag)
            for _ in range(3):
                if name == 'step':
                    _ok(lib.st_plan_lbfgs_step(plan.handle, x, state, ema, 0.99, losses, _stream()), tag)
                else:
                    _ok(lib.st_plan_loss_and_grad(plan.handle, x, grad, losses, _stream()), tag)
                    _ok(lib.st_lbfgs_update(state, n, x, grad, ema, 0.99, _stream()), tag)
                b.verify(tag)
            pairs.append({what: b.get(f'{what} {name}') for what in ('x', 'ema', 'losses')})
        for what in ('x', 'ema', 'losses'):
            assert torch.equal(pairs[0][what], pairs[1][what]), f'{tag}: {what}: st_plan_lbfgs_step differs from closure + update'
        assert not torch.equal(pairs[0]['x'], image.flatten()), tag
        out = {name: b.get(name) for name in b.bits()}
        out.update({f'feature {layer}': t.cpu() for layer, t in feats.items()})
        assert all(bool(torch.isfinite(t).all()) for t in out.values()), tag
        runs.append(out)
        del plan, net
    aligned, shifted = runs
    for name in aligned:
        if name.startswith(('feature', 'mean', 'srm')):
            assert torch.equal(aligned[name], shifted[name]), f'{size}: {name} depends on where the caller\'s buffer lies'
    # the moments against float64 moments of the plan's own tap (tests/test_kernels_gpu.py test_moments_of_taps, 1e-6)
    for layer in (1, 29):
        f = aligned[f'feature {layer}'][0].double().flatten(1)
        c = f.shape[0]
        for run in runs:
            assert rel_l2(run[f'srm {layer}'].view(c, c), (f @ f.t()) / f.shape[1]) <= 1e-6
            assert rel_l2(run[f'mean {layer}'], f.mean(1)) <= 1e-6
    _observe('st_plan_forward / _moments / _backward / _lbfgs_step', size, PLAN_SHIFTS[1], shifted, aligned)

# =====================================================================================================================
# 14. the modules on tensors that are dense but not 16-byte aligned (style_transfer/losses.py: eligible() takes them, _dense()
#     hands the library an aligned copy): value and gradient within the module tests' bar (1e-4) of the same module on a
#     clone, and the native counter shows that the native path ran
# =====================================================================================================================
MODULE_BAR = 1e-4


def _module_pair(module, kind, base, pick):
    """(value, gradient) of `module` on the misaligned view `pick(base)` and on an aligned clone of it."""
    from style_transfer import losses as L
    module = module.to(DEV)
    out = []
    for aligned in (False, True):
        leaf = (pick(base).detach().clone() if aligned else base.detach().clone()).requires_grad_(True)
        x = leaf if aligned else pick(leaf)
        assert x.is_contiguous() and (x.data_ptr() % 16 == 0) == aligned, (kind, x.data_ptr() % 16)
        before = L.native_calls.get(kind, 0)
        value = module(x)
        value.backward()
        _sync()
        assert L.native_calls.get(kind, 0) == before + 1, f'{kind}: the native path did not run (aligned={aligned})'
        grad = leaf.grad if aligned else pick(leaf.grad)
        assert torch.isfinite(value).all() and torch.isfinite(grad).all(), kind
        out.append((float(value.detach()), grad.detach().cpu().clone()))
    (v_off, g_off), (v_al, g_al) = out
    ev, eg = _rel(v_off, v_al), _gerr(g_off, g_al)
    print(f'[caller-buffers] module {kind}: misaligned view against an aligned clone: value {ev:.2e}, gradient {eg:.2e} (bar {MODULE_BAR:.0e})')
    assert ev <= MODULE_BAR and eg <= MODULE_BAR, (kind, ev, eg)


def test_image_and_content_modules_on_the_second_image_of_a_batch():
    """batch[1] of a [2, 3, 45, 54] tensor: dense fp32, 8 bytes past a 16-byte boundary; and a [64, 9, 13] tap one float off."""
    from style_transfer import losses as L
    g = torch.Generator().manual_seed(77)
    batch = torch.rand((2, 3, 45, 54), generator=g).to(DEV)
    other = torch.rand((3, 45, 54), generator=g).to(DEV)
    style = (1.3 * torch.randn((64, 9, 13), generator=g) + 0.2).to(DEV)
    assert batch[1].data_ptr() % 16 == 8
    tap = torch.randn((64 * 9 * 13 + 4,), generator=g).to(DEV)

    def second(t):
        return t[1]

    def shifted_tap(t):                      # a [64, 9, 13] tap one float past a 16-byte boundary
        return t[1:1 + 64 * 9 * 13].view(64, 9, 13)
    with L.native(True):
        _module_pair(L.TVLoss(), 'tv', batch, second)
        _module_pair(L.LaplacianLoss(other, pools=(1, 4)), 'laplacian', batch, second)
        _module_pair(L.ContentLossMSE(other), 'mse', batch, second)
        _module_pair(L.ContentLoss(other), 'scaled_mse', batch, second)
        _module_pair(L.StyleLossW2Diag(L.StyleLossW2Diag.get_target(style)), 'w2_diag', tap, shifted_tap)
        _module_pair(L.StyleLossW2Marginal(L.StyleLossW2Marginal.get_target(style)), 'w2_marginal', tap, shifted_tap)


def test_style_modules_on_a_view_one_float_off():
    """buf[1:1 + n].view(C, H, W): the standalone heads demand a 16-byte aligned tap, the modules hand them a copy."""
    from style_transfer import losses as L
    c, h, w = 64, 9, 13
    g = torch.Generator().manual_seed(78)
    buf = torch.randn((c * h * w + 4,), generator=g).to(DEV)
    style = (1.3 * torch.randn((1, c, h, w + 3), generator=g) + 0.2).to(DEV)

    def view(t):
        return t[1:1 + c * h * w].view(c, h, w)
    with L.native(True):
        _module_pair(L.StyleLossW2(L.StyleLossW2.get_target(style)), 'w2', buf, view)
        _module_pair(L.StyleLoss(L.StyleLoss.get_target(style)), 'gram', buf, view)
        _module_pair(L.StyleLossNearest(L.StyleLossNearest.get_target(style[0])), 'nearest', buf, view)
        _module_pair(L.StyleLossSliced(L.StyleLossSliced.get_target(style[0]), resample=False), 'sliced', buf, view)


# =====================================================================================================================
# 15. the option setters that read caller memory: st_plan_set_style_quantiles, _vectors, _sliced_vectors, _regions and
#     st_plan_set_content_target_at, fed from fenced buffers at offsets 0 to 3 - the plan must be the same plan, bit for bit
# =====================================================================================================================
OPTION_FLAGS = [True, False, False, True, True]       # relu1_1 (64 x 1920 at 40 x 48), relu4_1 (512 x 30), relu5_1 (512 x 6)


def _option_plan(option, shift):
    import test_taps_gpu as T
    hip, lib = _hip(), _lib()
    size = (40, 48)
    tag = f'{option} setters, shift {shift}'
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *size)
    flagged = OPTION_FLAGS if option in ('quantiles', 'vectors', 'sliced') else [False] * 5
    if option == 'quantiles':
        plan.set_w2_marginal(flagged)
    elif option == 'vectors':
        plan.set_style_nearest(flagged)
    elif option == 'sliced':
        plan.set_style_sliced(flagged)
        for i, flag in enumerate(flagged):
            if flag:
                plan.set_sliced_options(i, None, False)
    plan.set_loss_weights(*T._layer_weights(*T.DEFAULT), T.TV_WEIGHT)
    ctargets, moments = T._targets(size, 'max', *T.DEFAULT)
    sfeats = T._inputs(size, 'max')['sfeats']
    b = Buffers()
    _ok(lib.st_plan_set_content_target_at(plan.handle, 0, b.inp('content target', ctargets[22], shift), _stream()), tag)
    if option == 'regions':
        h, w = size
        left = torch.zeros((h, w))
        left[:, :w // 2 + 3] = 1.0
        masks = (ctypes.c_void_p * 2)(b.inp('region 0', left, shift).value, b.inp('region 1', (1.0 - 0.75 * left).contiguous(), shift).value)
        _ok(lib.st_plan_set_style_regions(plan.handle, 2, masks, _stream()), tag)
    for i, layer in enumerate(T.DEFAULT[1]):
        feat = sfeats[layer][0].flatten(1).contiguous()
        if not flagged[i]:
            for region in ((0, 1) if option == 'regions' else (0,)):
                _ok(lib.st_plan_set_region_style_target(plan.handle, region, i, b.inp(f'mean {layer} {region}', moments[layer][0], shift),
                                                        b.inp(f'srm {layer} {region}', moments[layer][1], shift), _stream()), tag)
        elif option == 'quantiles':
            q = torch.sort(feat + 0.0, dim=1, stable=True).values.contiguous()
            _ok(lib.st_plan_set_style_quantiles(plan.handle, i, b.inp(f'quantiles {layer}', q, shift), q.shape[1], _stream()), tag)
        elif option == 'vectors':
            _ok(lib.st_plan_set_style_vectors(plan.handle, i, b.inp(f'vectors {layer}', feat, shift), feat.shape[1], _stream()), tag)
        else:
            half = feat[:, :max(1, feat.shape[1] // 2)].contiguous()
            ptrs = (ctypes.c_void_p * 2)(b.inp(f'vectors {layer} a', feat, shift).value, b.inp(f'vectors {layer} b', half, (shift + 1) % 4).value)
            ms = (ctypes.c_longlong * 2)(feat.shape[1], half.shape[1])
            ws = (ctypes.c_float * 2)(0.25, 0.75)
            _ok(lib.st_plan_set_style_sliced_vectors(plan.handle, i, 2, ptrs, ms, ws, _stream()), tag)
    b.verify(tag)
    return net, plan, b


@pytest.mark.parametrize('option', ['quantiles', 'vectors', 'sliced', 'regions'])
def test_plan_option_setters_read_shifted_memory(option):
    import test_taps_gpu as T
    image = T._inputs((40, 48), 'max')['image']
    base = None
    for shift in (0, 1, 2, 3):
        net, plan, keep = _option_plan(option, shift)
        tag = f'{option} setters, shift {shift}'
        b, ptrs = _closure_buffers(image, PLAN_SHIFTS[0])
        first = _run_closure(plan, b, ptrs, tag)
        _same_bits(tag, first, _run_closure(plan, b, ptrs, tag))
        keep.verify(tag)
        got = {'grad': b.get('grad'), 'losses': b.get('losses')}
        assert bool((got['losses'] != 0).all()), (tag, got['losses'])          # every term is live
        base = base or got
        assert torch.equal(got['grad'], base['grad']) and torch.equal(got['losses'], base['losses']), \
            f'{tag}: a setter fed from a buffer off alignment gives another plan'
        del plan, net
