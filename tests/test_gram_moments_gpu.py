"""The Gram moment kernels (csrc/st_gram.hip) alone, at the sizes where their split of the pixel range saturates.

Every case runs ``Head('moments', C, h, w, DEV, precision).moments(feat)`` - gram_partial_kernel<false> (fp32),
gram_partial_f16_kernel<false> and gram_partial_f16_wide_kernel<false> (fp16x3, with the bound the head measures itself), then
gram_finalize_kernel - and first asserts the split plan it claims through st_op_gram_split_plan, so a later change of the
heuristic fails loudly instead of emptying the case.

a. exact count: small-integer features make every product, partial and total an integer below 2^23, exact in fp32 and in the
   fp16 planes - a pixel dropped, doubled or read from a neighbouring row at any boundary changes an integer;
b. rounding: post-ReLU features over 8 binades of channel scales, some channels with mean / std of about 30, against float64,
   by rel_l2 (MOMENT_TOL) and per entry, the bar taken from the fp32 CPU computation of the same inputs; a 12-decade input by
   rel_l2 alone (the price of one global fp16x3 scale);
c. structure: exact symmetry, run-to-run bits, a reused workspace, ST_XCD_REMAP=0.

The two tests without the gpu mark need no device: the split plans of every case, and the CPU emulation of the fp16x3 split
that the per-entry bar of (b) rests on.  Measured figures: profiles/gram_moments.md."""
import functools
import math

import numpy as np
import pytest
import torch

from conftest import rel_l2

gpu = pytest.mark.gpu
DEV = 'cuda:0'
MOMENT_TOL = 1e-6               # tests/test_native_losses_gpu.py, test_moments_of_taps
PRECISIONS = ('fp32', 'fp16x3')
RELU_STD = math.sqrt(0.5 - 0.5 / math.pi)       # std of relu(randn)
SPREAD_BINADES = 8              # channel scales 2^u, u uniform in [-8, 0]: what the emulation test found inside the bar


def _hip():
    from style_transfer import _hip
    return _hip


# (C, h, w, ST_GRAM_WIDE or None) -> {precision: (splits, per_split, wide)}.  The last pixels: see _tail.
CASES = {
    # the 768 / tiles cap: the rounded per_split leaves split 757 with 76 pixels and 758-767 empty
    'c64-250x400': ((64, 250, 400, None), {'fp32': (768, 132, False), 'fp16x3': (768, 132, False)}),
    # same cap, N % 4 = 1: every load takes the scalar path; split 758 holds 93 pixels, 759-767 none
    'c64-251x399': ((64, 251, 399, None), {'fp32': (768, 132, False), 'fp16x3': (768, 132, False)}),
    # the shipped 512^2 relu1_1 tap: split 762 holds 16 pixels, 763-767 none
    'c64-512x512': ((64, 512, 512, None), {'fp32': (768, 344, False), 'fp16x3': (768, 344, False)}),
    # 250 full splits, 250-255 empty, none partial
    'c128-165x200': ((128, 165, 200, None), {'fp32': (256, 132, False), 'fp16x3': (256, 132, False)}),
    # the last split holds 2 pixels
    'c256-70x139': ((256, 70, 139, None), {'fp32': (77, 128, False), 'fp16x3': (77, 128, False)}),
    # the wide kernel where it is chosen: split 254 holds 9 pixels, 255 none (fp32: the same split, 64 x 64 tiles)
    'c256-257x257': ((256, 257, 257, None), {'fp32': (256, 260, False), 'fp16x3': (256, 260, True)}),
    'c256-257x257-narrow': ((256, 257, 257, 0), {'fp32': (77, 860, False), 'fp16x3': (77, 860, False)}),
    # wide, 10 tile pairs: 768 / 10 = 77 wanted, but a 512-channel head's workspace holds 64 partials (head_gram_split_cap)
    'c512-257x257': ((512, 257, 257, None), {'fp32': (64, 1036, False), 'fp16x3': (64, 1036, True)}),
    # both sides of the finalize kernel's 8 thread groups and of its 4-way unrolled loop (k + 24 < splits)
    'c64-1x1': ((64, 1, 1, None), {'fp32': (1, 4, False), 'fp16x3': (1, 4, False)}),
    'c64-1x100': ((64, 1, 100, None), {'fp32': (1, 100, False), 'fp16x3': (1, 100, False)}),
    'c64-1x129': ((64, 1, 129, None), {'fp32': (2, 68, False), 'fp16x3': (2, 68, False)}),
    'c64-1x897': ((64, 1, 897, None), {'fp32': (8, 116, False), 'fp16x3': (8, 116, False)}),
    'c64-1x1025': ((64, 1, 1025, None), {'fp32': (9, 116, False), 'fp16x3': (9, 116, False)}),
    'c64-1x3100': ((64, 1, 3100, None), {'fp32': (25, 124, False), 'fp16x3': (25, 124, False)}),
    'c64-1x4200': ((64, 1, 4200, None), {'fp32': (33, 128, False), 'fp16x3': (33, 128, False)}),
    # one split, below one LDS stage
    'c512-5x6': ((512, 5, 6, None), {'fp32': (1, 32, False), 'fp16x3': (1, 32, False)}),
    # the wide kernel forced onto a ragged tap
    'c128-45x37-forced': ((128, 45, 37, 2), {'fp32': (14, 120, False), 'fp16x3': (14, 120, True)}),
}
# case -> (index of the last split that holds pixels, its pixels, empty splits behind it)
TAILS = {
    'c64-250x400': (757, 76, 10), 'c64-251x399': (758, 93, 9), 'c64-512x512': (762, 16, 5), 'c128-165x200': (249, 132, 6),
    'c256-70x139': (76, 2, 0), 'c256-257x257': (254, 9, 1), 'c256-257x257-narrow': (76, 689, 0), 'c512-257x257': (63, 781, 0),
    'c64-1x1': (0, 1, 0), 'c64-1x100': (0, 100, 0), 'c64-1x129': (1, 61, 0), 'c64-1x897': (7, 85, 0), 'c64-1x1025': (8, 97, 0),
    'c64-1x3100': (24, 124, 0), 'c64-1x4200': (32, 104, 0), 'c512-5x6': (0, 30, 0), 'c128-45x37-forced': (13, 105, 0),
}
STALE_CASES = ('c64-250x400', 'c256-257x257')
EMULATED_CASE = 'c64-250x400'


def _shape(case):
    c, h, w, _ = CASES[case][0]
    return c, h, w, h * w


def _switches(case):
    wide = CASES[case][0][3]
    return {} if wide is None else {'ST_GRAM_WIDE': wide}


def _tail(npix, splits, per_split):
    last = (npix - 1) // per_split
    return last, npix - last * per_split, splits - 1 - last


def _assert_plan(case, precision):
    """The regime the case claims, from the library's own answer for the shape (under the case's switches)."""
    hip = _hip()
    c, _, _, n = _shape(case)
    plan = hip.gram_split_plan(c, n, precision)
    assert plan == CASES[case][1][precision], f'{case} {precision}: the split plan is now {plan}'
    splits, per_split, _ = plan
    assert per_split % 4 == 0 and splits * per_split >= n
    assert _tail(n, splits, per_split) == TAILS[case], f'{case}: the last splits are now {_tail(n, splits, per_split)}'
    return plan


# ---- inputs and float64 references: made once per module, never written to ------------------------------------------------------
def _seed(kind, c, n):
    return {'int': 1, 'relu': 2, 'decades': 3}[kind] * 1000003 + c * 4099 + n


def _special_channels(c):
    return 37, c - 6          # all zero, constant 1: in different 32-row blocks, and in different tiles where there are several


@functools.lru_cache(maxsize=None)
def _input(kind, c, n):
    g = torch.Generator().manual_seed(_seed(kind, c, n))
    if kind == 'int':
        f = torch.randint(-4, 5, (c, n), generator=g).float()
        zero, one = _special_channels(c)
        f[zero] = 0.
        f[one] = 1.
        return f
    f = torch.relu(torch.randn((c, n), generator=g))
    if kind == 'relu':
        scale = torch.exp2(-SPREAD_BINADES * torch.rand((c, 1), generator=g))
        f = f * scale
        f[3::8] += 30. * RELU_STD * scale[3::8]           # mean / std of about 30 in every 8th channel
        return f
    return f * torch.logspace(-8, 4, c).reshape(c, 1)     # 'decades': channels spanning 12 decades


@functools.lru_cache(maxsize=None)
def _reference(kind, c, n):
    """float64 F F^T / N and F 1 / N - for 'int' the exact integer sums instead - and the fp32 CPU computation's per-entry
    figures against them."""
    f = _input(kind, c, n)
    f64 = f.double()
    gram, rows = f64 @ f64.t(), f64.sum(1)
    if kind == 'int':
        return gram, rows
    srm, mean = gram / n, rows / n
    srm32 = torch.einsum('cn,dn->cd', f, f) / n
    mean32 = f.sum(1) / n
    return srm, mean, _per_entry(srm32, mean32, srm, mean)


def _per_entry(srm, mean, want_srm, want_mean):
    """(max_ij |srm - want| / sqrt(want_ii want_jj), max_i |mean - want| / sqrt(want_ii)).  Where a channel is identically zero
    (want_ii = 0) the result must be exactly zero too; those entries take no part in the maximum."""
    srm, mean = srm.detach().cpu().double(), mean.detach().cpu().double()
    d = want_srm.diagonal().sqrt()
    dd = d[:, None] * d[None, :]
    live, live_c = dd > 0, d > 0
    assert not srm[~live].any() and not mean[~live_c].any(), 'a channel without energy has non-zero moments'
    es = float(((srm - want_srm).abs()[live] / dd[live]).max()) if live.any() else 0.
    em = float(((mean - want_mean).abs()[live_c] / d[live_c]).max()) if live_c.any() else 0.
    return es, em


def _moments(case, precision, feat, head=None):
    hip = _hip()
    c, h, w, _ = _shape(case)
    with hip.options(**_switches(case)):
        head = head or hip.Head('moments', c, h, w, DEV, precision)
        mean, srm = head.moments(feat)
    torch.cuda.synchronize()
    return mean, srm, head


def _dev(kind, case):
    c, h, w, n = _shape(case)
    return _input(kind, c, n).to(DEV).reshape(c, h, w)


# ---- no device: the plans, and what the fp16x3 split alone costs per entry -----------------------------------------------------
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_split_plan_of_every_case(case, precision):
    hip = _hip()
    with hip.options(**_switches(case)):
        _assert_plan(case, precision)


def test_split_plan_refuses_what_a_head_refuses():
    hip = _hip()
    for c, n, precision in ((96, 1000, 'fp32'), (64, 0, 'fp32'), (64, hip.max_pixels() + 1, 'fp16x3'), (64, 1000, 'bf16x3')):
        with pytest.raises(hip.HipLibraryError):
            hip.gram_split_plan(c, n, precision)
    assert hip.gram_split_plan(64, hip.max_pixels(), 'fp32')[0] == 768


def _fp16x3_emulation(f):
    """The fp16x3 pass on the CPU: the power-of-two scale of scale_exp (st_common.h) from max |f|, the two fp16 planes of
    split_store, the three products - summed in float64, so what is left is the split's own error."""
    amax = np.float32(f.abs().max())
    ef = (int(amax.view(np.uint32)) >> 23) & 0xff
    ex = 14 - (ef - 126)
    x = (f.numpy() * np.float32(2.0 ** ex)).astype(np.float32)
    h0 = x.astype(np.float16)
    h1 = (x - h0.astype(np.float32)).astype(np.float16)
    assert np.isfinite(h0).all()
    a, b = torch.from_numpy(h0.astype(np.float64)), torch.from_numpy(h1.astype(np.float64))
    cross = a @ b.t()
    return (a @ a.t() + cross + cross.t()) * 4.0 ** -ex / f.shape[1]


def test_fp16x3_emulation_stays_inside_the_per_entry_bar():
    """Before (b) holds the fp16x3 kernels to the per-entry bar: the two-plane split by itself, with exact sums, must meet it at
    this spread of channel scales."""
    c, _, _, n = _shape(EMULATED_CASE)
    f = _input('relu', c, n)
    srm, mean, (ref_s, _) = _reference('relu', c, n)
    es, _ = _per_entry(_fp16x3_emulation(f), mean, srm, mean)
    bar = max(1e-6, 4 * ref_s)
    print(f'[gram-moments] emulation {EMULATED_CASE} spread 2^-{SPREAD_BINADES}: per-entry srm {es:.3e} '
          f'(fp32 CPU {ref_s:.3e}, bar {bar:.3e}); rel_l2 {rel_l2(_fp16x3_emulation(f), srm):.3e}')
    assert es <= bar


# ---- a. exact count --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_exact_count(case, precision):
    """Features in {-4 .. 4}, one channel zero, one constant 1: N srm and N mean are the integer sums, exactly."""
    hip = _hip()
    with hip.options(**_switches(case)):
        plan = _assert_plan(case, precision)
    c, _, _, n = _shape(case)
    f = _input('int', c, n)
    gram, rows = _reference('int', c, n)
    # the precondition: every partial sum, in any order, is an integer below 2^23 (16 N at most)
    bound = float((f.abs().double() @ f.abs().double().t()).max())
    assert bound < 2 ** 23 and float(f.abs().sum(1).max()) < 2 ** 23 and 16 * n < 2 ** 23
    mean, srm, _ = _moments(case, precision, _dev('int', case))
    mean, srm = mean.cpu().double(), srm.cpu().double()
    wrong = (srm * n).round() != gram
    wrong_rows = (mean * n).round() != rows
    zero, one = _special_channels(c)
    eq = (float(srm[one, one]) == 1.0, float(mean[one]) == 1.0)
    print(f'[gram-moments] exact {case} {precision} plan {plan}: {int(wrong.sum())} of {c * c} sums and {int(wrong_rows.sum())} '
          f'of {c} row sums differ; constant channel srm == 1: {eq[0]}, mean == 1: {eq[1]}')
    assert not wrong.any(), f'{int(wrong.sum())} entries of N srm are not the integer Gram, first at {wrong.nonzero()[0].tolist()}: ' \
                            f'{float((srm * n)[tuple(wrong.nonzero()[0])])} vs {float(gram[tuple(wrong.nonzero()[0])])}'
    assert not wrong_rows.any(), f'row sums differ at channels {wrong_rows.nonzero().flatten().tolist()[:8]}'
    assert not srm[zero].any() and not srm[:, zero].any() and float(mean[zero]) == 0.
    ulp = 2.0 ** -23
    assert abs(float(srm[one, one]) - 1.0) <= ulp and abs(float(mean[one]) - 1.0) <= ulp


# ---- b. rounding -----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_rounding_against_float64(case, precision):
    hip = _hip()
    with hip.options(**_switches(case)):
        plan = _assert_plan(case, precision)
    c, _, _, n = _shape(case)
    want_srm, want_mean, (ref_s, ref_m) = _reference('relu', c, n)
    mean, srm, _ = _moments(case, precision, _dev('relu', case))
    rs, rm = rel_l2(srm.cpu(), want_srm), rel_l2(mean.cpu(), want_mean)
    es, em = _per_entry(srm, mean, want_srm, want_mean)
    bar_s, bar_m = max(1e-6, 4 * ref_s), max(1e-6, 4 * ref_m)
    print(f'[gram-moments] rounding {case} {precision} plan {plan}: rel_l2 srm {rs:.3e} mean {rm:.3e}; per-entry srm {es:.3e} '
          f'(fp32 CPU {ref_s:.3e}, bar {bar_s:.3e}) mean {em:.3e} (fp32 CPU {ref_m:.3e}, bar {bar_m:.3e})')
    assert rs <= MOMENT_TOL and rm <= MOMENT_TOL
    assert es <= bar_s and em <= bar_m


@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_twelve_decades_of_channel_scales(case, precision):
    """One global power-of-two scale serves all channels: the quiet ones lose per-entry accuracy in fp16x3 (documented, printed),
    the result as a whole keeps the bar and stays finite."""
    c, _, _, n = _shape(case)
    want_srm, want_mean, (ref_s, ref_m) = _reference('decades', c, n)
    mean, srm, _ = _moments(case, precision, _dev('decades', case))
    assert torch.isfinite(srm).all() and torch.isfinite(mean).all()
    rs, rm = rel_l2(srm.cpu(), want_srm), rel_l2(mean.cpu(), want_mean)
    srm, mean = srm.cpu().double(), mean.cpu().double()
    d = want_srm.diagonal().sqrt()
    live = d > 0
    es = float(((srm - want_srm).abs() / (d[:, None] * d[None, :]))[live][:, live].max())
    em = float(((mean - want_mean).abs() / d)[live].max())
    print(f'[gram-moments] decades {case} {precision}: rel_l2 srm {rs:.3e} mean {rm:.3e}; per-entry srm {es:.3e} '
          f'(fp32 CPU {ref_s:.3e}) mean {em:.3e} (fp32 CPU {ref_m:.3e})')
    assert rs <= MOMENT_TOL and rm <= MOMENT_TOL


# ---- c. structure ----------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', list(CASES))
def test_symmetry_and_bits(case, precision):
    hip = _hip()
    feat = _dev('relu', case)
    mean, srm, head = _moments(case, precision, feat)
    assert torch.equal(srm, srm.t()), 'second raw moment must be exactly symmetric'
    mean2, srm2, _ = _moments(case, precision, feat, head)
    assert torch.equal(srm, srm2) and torch.equal(mean, mean2), 'two calls on one head differ'
    with hip.options(ST_XCD_REMAP=0):
        mean3, srm3, _ = _moments(case, precision, feat)
    assert torch.equal(srm, srm3) and torch.equal(mean, mean3), 'ST_XCD_REMAP=0 changes the bits'


@gpu
@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('case', STALE_CASES)
def test_reused_workspace_is_overwritten(case, precision):
    """A head that ran input A and then B returns B's moments as a fresh head does: the empty and short splits of the grid write
    their partials too."""
    a, b = _dev('relu', case) * 64., _dev('int', case)
    _, _, head = _moments(case, precision, a)
    mean, srm, _ = _moments(case, precision, b, head)
    want_mean, want_srm, _ = _moments(case, precision, b)
    assert torch.equal(srm, want_srm) and torch.equal(mean, want_mean)
    c, _, _, n = _shape(case)
    gram, rows = _reference('int', c, n)
    assert torch.equal((srm.cpu().double() * n).round(), gram) and torch.equal((mean.cpu().double() * n).round(), rows)
