"""Cosine and centred-cosine matching of a nearest head (st_plan_set_nearest_metric, the st_op_nearest_cosine_* entries,
StyleTransfer.style_nearest_metric, losses.StyleLossNearest(metric=...)) on a real MI355X.

Formula (include/st_amd.h), written out in float64 below, eps = 1e-8:
    mu = 0 ('cosine') or the mean of the style vectors, rounded to fp32 ('centered_cosine');
    s^_k = (s_k - mu) / sqrt(|s_k - mu|^2 + eps);  g_i = f_i - mu;  p_i(k) = <g_i, s^_k>;  r_i = sqrt(|g_i|^2 + eps);
    k*(i) = argmax_k p_i(k), ties: the lowest k;  term = sum_i (1 - p_i(k*) / r_i) / N;  dF = (1 / N) (-s^_k* / r_i + p_i(k*) g_i / r_i^3).

How a match is judged.  Planted matches - f_i = mu + 0.05 (s_pi(i) - mu): the cosine to the planted vector is 1, to every other
one far less, while under L2 such a SHORT vector is nearest to whichever style vector is shortest - must be found exactly, and
the test shows on its own data that the L2 arg-min is somewhere else on most pixels, so a metric that is ignored cannot pass.
On unrelated data the search may legitimately pick either of two near-equal vectors, so the DEFICIT of the chosen one is bounded,
    deficit_i = p64_i(k_best) - p64_i(k_gpu),      p64_i(k) = <f_i - mu, s^_k> in float64, s^_k the UNROUNDED unit vector,
by a bound derived from the search's arithmetic, not from what it returns.  The search compares score(i, k) = <f_i, s^_k> + b_k
with the fp32 rows s^ and b_k = -<mu, s^_k> the setter prepared; if E_i bounds |computed score - p64_i(k)| for every k, the chosen
vector's p64 is at most 2 E_i below the best one's.  Names: aF = max |F_ci| (elements), nf_i = |f_i|, nmu = |mu| (vector norms);
max |s^_ck| <= 1 and |s^_k| <= 1 stand where tests/test_style_nearest_gpu.py has max |S| and max_k |s_k|.  E_i has five parts:
  * the rows are rounded to fp32 once: |s^32 - s^64| <= 2^-24 |s^64| per element, so <f_i, s^_k> moves by at most 2^-24 nf_i
    and b_k by at most 2^-24 nmu;
  * operands (the derivation of tests/test_style_nearest_gpu.py with the rows' bound B <= 2 max |s^| <= 2): per channel
    2^-23 + 2^-23 + 2^-22 = 2^-21 times aF, (C + 1) 2^-21 aF over the channels;
  * accumulation: 3 C fp32 additions of partial sums that are at most sum_c |f_c s^_c| <= nf_i: 3 C 2^-24 nf_i;
  * b_k is summed in double and rounded to fp32 once: 2^-25 |b_k| <= 2^-25 nmu;
  * the final addition of the bias rounds by 2^-24 |score| <= 2^-24 (nf_i + nmu).
  E_i = (C + 1) 2^-21 aF + (3 C + 2) 2^-24 nf_i + 3 2^-24 nmu, and the bar is deficit_i <= 2 E_i for EVERY pixel, in this absolute
form so that an all-zero tap is judged too.  The largest measured deficit over its bar is printed.

Values and gradients are judged against the float64 formula evaluated WITH THE KERNEL'S INDICES at the project's bars for
standalone operators: 1e-4 relative on the value, 1e-4 rel-L2 on the gradient (the finish pass recomputes p_i and |g_i|^2 in fp32;
it never takes the search's score).

Plans: inputs and helpers are tests/test_style_nearest_gpu.py's: sizes 40 x 48 and 45 x 54, the oracle composed in float64 on the
plan's own ReLU and pool decisions with the plan's matches held constant.  Every flagged term within 1e-4 of float64, every
image gradient within 1e-4 rel-L2 of float64.  A metric that is ignored or mixed up cannot pass: on every flagged layer the other
two metrics' terms of the same tap, each at its own float64 matches, lie at least 10 bars from the tested one.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_l2
import st_oracle as O
import test_content_tv_masks_gpu as CM
import test_laplacian_gpu as LG
import test_layer_losses_gpu as L
import test_loss_kinds_gpu as K
import test_style_mask_gpu as MG
import test_style_nearest_gpu as NG
import test_taps_gpu as T
import test_w2_diagonal_gpu as D
from test_laplacian_cpu import formula_terms

pytestmark = pytest.mark.gpu
DEV = T.DEV
SIZE, ODD = D.SIZE, D.ODD
ALL, DEEP, MSE, W2 = D.ALL, D.DEEP, D.MSE, D.W2
NONE = [False] * 5
IGNORED_BARS = NG.IGNORED_BARS
BAR = 1e-4
EPS = 1e-8
METRICS = ('cosine', 'centered_cosine')


# ---- the float64 side ---------------------------------------------------------------------------------------------------------
def _parts(s, metric):
    """(mu [C], the unrounded unit vectors [C, M]) in float64 for the style vectors s [C, M] fp32 on the CPU."""
    s64 = s.double()
    mu = s64.mean(1).float().double() if metric == 'centered_cosine' else torch.zeros(s.shape[0], dtype=torch.float64)
    d = s64 - mu[:, None]
    return mu, d / torch.sqrt((d * d).sum(0) + EPS)


def _scores(f, mu, unit):
    """p64 [N, M]."""
    return (f.double() - mu[:, None]).T @ unit


def _first_argmax(p):
    top = p.max(dim=1, keepdim=True).values
    return torch.where(p == top, torch.arange(p.shape[1])[None, :], p.shape[1]).min(dim=1).values


def _deficit_bars(f, mu):
    """2 E_i of the header for every pixel."""
    c = f.shape[0]
    a_f, nf, nmu = float(f.double().abs().max()), f.double().norm(dim=0), float(mu.norm())
    return 2.0 * ((c + 1) * 2.0 ** -21 * a_f + (3 * c + 2) * 2.0 ** -24 * nf + 3 * 2.0 ** -24 * nmu)


def _check_deficit(tag, f, s, metric, k):
    """The deficit check of the header on every pixel; returns the largest deficit over its bar."""
    assert k.dtype == torch.int64 and k.shape == (f.shape[1],) and int(k.min()) >= 0 and int(k.max()) < s.shape[1], tag
    mu, unit = _parts(s, metric)
    p = _scores(f, mu, unit)
    deficit = p.max(dim=1).values - p.gather(1, k[:, None])[:, 0]
    bars = _deficit_bars(f, mu)
    slack = 1e-12 * (float(f.double().norm(dim=0).max()) + float(mu.norm()) + 1.0)      # (p64 itself is a float64 sum)
    worst = float((deficit / bars.clamp(min=1e-300)).max())
    print(f'[nearest-cosine] {tag} {metric}: largest deficit {float(deficit.max()):.3e}, largest deficit / its bar {worst:.3e}')
    assert bool((deficit <= bars + slack).all()), f'{tag} {metric}: a deficit above 2 E_i: {float((deficit - bars).max()):.3e}'
    return worst


def _formula(f, s, metric, k):
    """(term, dF) at weight 1 in float64 for the matches k."""
    mu, unit = _parts(s, metric)
    g = f.double() - mu[:, None]
    sel = unit[:, k]
    p = (g * sel).sum(0)
    r = torch.sqrt((g * g).sum(0) + EPS)
    n = f.shape[1]
    return float((1.0 - p / r).sum() / n), (-sel / r + p * g / r ** 3) / n


# ---- 1. the standalone entries --------------------------------------------------------------------------------------------------
def _shapes():
    from style_transfer import _hip as hip
    chunk, tpx, tk = hip.nearest_geometry()
    split = 4 * tk                      # the k range of one split at these pixel counts (st_op_nearest_splits)
    shapes = [(2 * chunk, 1, 1), (2 * chunk, tpx - 1, tk - 1), (2 * chunk, tpx, tk), (2 * chunk, tpx + 1, tk + 1),
              (2 * chunk, 300, 257), (2 * chunk, 130, split - 1), (2 * chunk, 257, split), (2 * chunk, 70, split + 1),
              (2 * chunk, 100, 2 * split), (2 * chunk, 100, 2 * split + 1), (512, 513, 1025), (128, 257, 4099), (512, 1, 1)]
    assert [hip.nearest_splits(n, m) for _, n, m in shapes] == [1, 1, 1, 1, 1, 1, 1, 2, 2, 3, 3, 9, 1]
    # one channel chunk; five chunks (a pixel's sums cross a channel group that is not full); one below, at and above a finish tile
    return shapes + [(32, 65, 129), (160, 130, 300), (64, 63, 200), (64, 64, 200), (64, 65, 200)]


N_SHAPES = 18
_gauss = NG._gauss


def _prepare(s, metric):
    from style_transfer import _hip as hip
    return hip.op_nearest_cosine_prepare(s.to(DEV), centered=metric == 'centered_cosine')


def _prepared_views(prepared, c, m):
    """(bias [M_pad], rows [M_pad, C], mu [C]) of a prepared buffer, from its end (the bound's words lie in front)."""
    m_pad, pad = (m + 127) // 128 * 128, (c + 63) // 64 * 64
    body = prepared[:prepared.numel() - pad]
    return body[-m_pad * (c + 1):-m_pad * c], body[-m_pad * c:].view(m_pad, c), prepared[prepared.numel() - pad:][:c]


@pytest.mark.parametrize('index', (1, 4, 9, 13, 14))
def test_the_prepared_set_is_the_headers(index):
    from style_transfer import _hip as hip
    c, _, m = _shapes()[index]
    lib = hip.load_library()
    assert lib.st_op_nearest_cosine_prepared_floats(c, m) == lib.st_op_nearest_prepared_floats(c, m) + (c + 63) // 64 * 64
    for metric in METRICS:
        s = _gauss(c, m, 500 + index, relu=True)
        s[:, m // 2] = 0                                                      # a zero vector stays zero (metric 'cosine')
        prepared = _prepare(s, metric)
        torch.cuda.synchronize()
        assert prepared.numel() == lib.st_op_nearest_cosine_prepared_floats(c, m)
        bias, rows, mu = (t.cpu() for t in _prepared_views(prepared, c, m))
        want_mu, unit = _parts(s, metric)
        assert torch.equal(mu.double(), want_mu) or float((mu.double() - want_mu).abs().max()) <= 2.0 ** -23 * float(want_mu.abs().max())
        assert float((rows[:m].double() - unit.T).abs().max()) <= 2.0 ** -23 and not rows[m:].any()
        assert float(rows.abs().max()) <= 1.0
        want_b = -(mu.double()[None, :] * rows[:m].double()).sum(1)
        assert float((bias[:m].double() - want_b).abs().max()) <= 2.0 ** -23 * max(float(want_b.abs().max()), 1e-30)
        assert bool(torch.isneginf(bias[m:]).all())
        if metric == 'cosine':
            assert not mu.any() and not bias[:m].any() and not rows[m // 2].any()


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_planted_scaled_matches_are_found_exactly(index):
    from style_transfer import _hip as hip
    c, n, m = _shapes()[index]
    for relu in (False, True):
        g = torch.Generator().manual_seed(1000 + 2 * index + relu)
        s = _gauss(c, m, 2000 + 2 * index + relu, relu)
        perm = torch.randint(0, m, (n,), generator=g)
        for metric in METRICS:
            mu, unit = _parts(s, metric)
            f = (mu[:, None] + 0.05 * (s.double()[:, perm] - mu[:, None])).float().contiguous()
            if m > 1:
                # the data's own properties: the planted vector is the float64 cosine arg-max by a margin of at least 0.16 r_i
                # (the largest bar 2 E_i is below 0.004 r_i at these shapes), and the L2 arg-min is somewhere else on most
                # pixels (91 % and more) - so a metric that is ignored cannot pass
                p = _scores(f, mu, unit)
                assert torch.equal(_first_argmax(p), perm)
                r = torch.sqrt(((f.double() - mu[:, None]) ** 2).sum(0) + EPS)
                runner_up = p.scatter(1, perm[:, None], -float('inf')).max(dim=1).values
                assert float(((p.gather(1, perm[:, None])[:, 0] - runner_up) / r).min()) >= 0.16
                l2 = NG._distances(f, s)[1]
                elsewhere = float((l2 != perm).double().mean())
                print(f'[nearest-cosine] planted ({c}, {n}, {m}) relu={relu} {metric}: the L2 arg-min differs on {100 * elsewhere:.0f} %')
                assert elsewhere >= 0.5
            prepared = _prepare(s, metric)
            _, _, k = hip.op_nearest_cosine_loss(f.to(DEV), prepared, m)
            ks, _ = hip.op_nearest_search(f.to(DEV), prepared, m)              # the search entry serves all three metrics
            torch.cuda.synchronize()
            assert torch.equal(k.cpu(), perm), f'({c}, {n}, {m}) relu={relu} {metric}: {int((k.cpu() != perm).sum())} of {n} planted matches missed'
            assert torch.equal(ks, k)


WORST = {}


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_unrelated_data_and_the_all_zero_tap(index):
    from style_transfer import _hip as hip
    c, n, m = _shapes()[index]
    for metric in METRICS:
        for relu in (False, True):
            f, s = _gauss(c, n, 3000 + 2 * index + relu, relu), _gauss(c, m, 4000 + 2 * index + relu, relu)
            _, _, k = hip.op_nearest_cosine_loss(f.to(DEV), _prepare(s, metric), m)
            WORST[(index, metric, relu)] = _check_deficit(f'unrelated ({c}, {n}, {m}) relu={relu}', f, s, metric, k.cpu())
        f, s = torch.zeros((c, n)), _gauss(c, m, 5000 + index)
        _, _, k = hip.op_nearest_cosine_loss(f.to(DEV), _prepare(s, metric), m)
        _check_deficit(f'all-zero tap ({c}, {n}, {m})', f, s, metric, k.cpu())
        if metric == 'cosine':                   # every score is the bias 0: the lowest index
            assert not k.any()
    print(f'[nearest-cosine] largest deficit / its bar so far: {max(WORST.values()):.3e}')


def test_ties_go_to_the_lowest_index():
    """Bit-identical duplicate columns in one k tile, in different tiles of one split and in different splits (four splits)."""
    from style_transfer import _hip as hip
    c, m = 64, 1600
    assert hip.nearest_splits(200, m) == 4 and hip.nearest_geometry() == (32, 128, 128)
    s = _gauss(c, m, 61)
    groups = [(3, 77), (5, 300), (9, 700, 1500), (130, 131), (600, 1100), (40, 511, 512, 1599)]
    for group in groups:
        for k in group[1:]:
            s[:, k] = s[:, group[0]]
    g = torch.Generator().manual_seed(62)
    owners = torch.tensor([group[i % len(group)] for i, group in enumerate(groups * 34)][:200])
    want = torch.tensor([group[0] for group in (groups * 34)][:200])
    for metric in METRICS:
        mu = _parts(s, metric)[0].float()
        f = (mu[:, None] + 0.05 * (s[:, owners] - mu[:, None]) + 1e-4 * torch.randn((c, 200), generator=g)).contiguous()
        _, _, k = hip.op_nearest_cosine_loss(f.to(DEV), _prepare(s, metric), m)
        assert torch.equal(k.cpu(), want), (metric, k.cpu()[k.cpu() != want], want[k.cpu() != want])
        # every column the same vector: index 0 everywhere, whatever the split
        same = s[:, :1].expand(c, m).contiguous()
        _, _, k = hip.op_nearest_cosine_loss(f.to(DEV), _prepare(same, metric), m)
        assert not k.any()


VALUE_WORST = {}


@pytest.mark.parametrize('index', range(N_SHAPES))
def test_value_gradient_determinism_and_the_module(index):
    from style_transfer import _hip as hip
    from style_transfer import losses
    c, n, m = _shapes()[index]
    for metric in METRICS:
        f = (_gauss(c, n, 80 + index, relu=True) * 1.5 - 0.1).contiguous()
        s = _gauss(c, m, 90 + index, relu=True)
        sd = s.to(DEV)
        prepared, prepared2 = _prepare(s, metric), _prepare(s, metric)
        # a tap pixel that is exactly zero ('cosine') or exactly mu ('centered_cosine'): the gradient there is -(1 / N) s^_k / sqrt(eps)
        mu_dev = _prepared_views(prepared, c, m)[2].cpu()
        special = n // 2
        f[:, special] = mu_dev
        fd = f.to(DEV)
        loss, unit, k = hip.op_nearest_cosine_loss(fd, prepared, m)
        loss2, unit2, k2 = hip.op_nearest_cosine_loss(fd, prepared2, m)
        up = torch.tensor(-1.75, device=DEV)
        grad_up = hip.op_nearest_loss_backward(unit, up)
        torch.cuda.synchronize()
        # two calls are equal in bits, indices included (of the prepared buffer the bias, the rows and mu are compared: of its
        # bound's slots only the largest exponent is ever read)
        tail = (m + 127) // 128 * 128 * (c + 1) + (c + 63) // 64 * 64
        assert torch.equal(prepared[-tail:], prepared2[-tail:])
        assert torch.equal(loss, loss2) and torch.equal(unit, unit2) and torch.equal(k, k2)
        _check_deficit(f'loss ({c}, {n}, {m})', f, s, metric, k.cpu())
        want, want_grad = _formula(f, s, metric, k.cpu())
        norm = float(want_grad.norm())
        ev = abs(loss.item() - want) / abs(want)
        if norm == 0.0:                         # one style vector, centred: s^ = 0 and the term is constant
            assert not unit.any() and not grad_up.any()
            eg = eu = es = 0.0
        else:
            eg = float((unit.cpu().double() - want_grad).norm()) / norm
            eu = float((grad_up.cpu().double() + 1.75 * want_grad).norm()) / (1.75 * norm)
            rows = _prepared_views(prepared, c, m)[1].cpu().double()
            at_zero = -rows[int(k[special])] / (n * EPS ** 0.5)
            es = float((unit.cpu().double()[:, special] - at_zero).norm()) / float(at_zero.norm())
            es = max(es, float((want_grad[:, special] - at_zero).norm()) / float(at_zero.norm()))
        print(f'[nearest-cosine] operators ({c}, {n}, {m}) {metric}: value {ev:.2e}, gradient {eg:.2e}, under upstream -1.75 {eu:.2e}, '
              f'at the pixel that equals mu {es:.2e} (bars 1e-4)')
        VALUE_WORST[(index, metric)] = (ev, eg, eu, es)
        assert ev <= BAR and eg <= BAR and eu <= BAR and es <= BAR
        assert 0.0 <= loss.item() <= 2.0
        # the module: the native path is counted under 'nearest_cosine', agrees with float64, and native(False) takes torch
        h = 1 if n < 4 or n % 4 else 4
        shape = (c, h, n // h)
        module = losses.StyleLossNearest(sd, metric)
        before, before_l2 = losses.native_calls.get('nearest_cosine', 0), losses.native_calls.get('nearest', 0)
        xn = fd.reshape(shape).clone().requires_grad_()
        value = module(xn)
        (value * 3.5).backward()
        assert losses.native_calls.get('nearest_cosine', 0) == before + 1 and losses.native_calls.get('nearest', 0) == before_l2
        assert abs(value.item() - want) / abs(want) <= BAR
        if norm:
            assert rel_l2(xn.grad.cpu().double().reshape(c, n), 3.5 * want_grad) <= BAR
        if index in (4, 9, 14):
            with losses.native(False):
                value_t = module(fd.reshape(shape))
            assert losses.native_calls.get('nearest_cosine', 0) == before + 1
            assert abs(value.item() - value_t.item()) / abs(value_t.item()) <= BAR
    print('[nearest-cosine] largest (value, gradient, upstream, zero pixel) so far: '
          + ', '.join(f'{max(v[i] for v in VALUE_WORST.values()):.2e}' for i in range(4)))


def test_the_module_on_the_device():
    from style_transfer import losses
    x = _gauss(64, 120, 21, relu=True).reshape(64, 12, 10).to(DEV)
    target = losses.StyleLossNearest.get_target(_gauss(64, 99, 22, relu=True).reshape(1, 64, 9, 11).to(DEV))[0]
    for metric in METRICS:
        module = losses.StyleLossNearest(target, metric)
        before = losses.native_calls.get('nearest_cosine', 0)
        # a batch, float64, a channel count that is no multiple of the K chunk and create_graph are the torch code
        assert torch.isfinite(module(torch.stack([x, x]))) and torch.isfinite(module.double()(x.double()))
        assert torch.isfinite(losses.StyleLossNearest(target[:48], metric)(x[:48]))
        module = module.float()
        assert losses.native_calls.get('nearest_cosine', 0) == before
        xg = x.clone().requires_grad_()
        (g,) = torch.autograd.grad(module(xg), xg, create_graph=True)
        assert losses.native_calls.get('nearest_cosine', 0) == before + 1 and g.requires_grad
        g.pow(2).sum().backward()
        assert torch.isfinite(xg.grad).all()
        with losses.native(False):
            fallback = module(x)
        assert losses.native_calls.get('nearest_cosine', 0) == before + 1
        native = module(x)
        assert losses.native_calls.get('nearest_cosine', 0) == before + 2
        assert abs(native.item() - fallback.item()) / abs(fallback.item()) <= BAR
        assert list(module.state_dict()) == ['target']
    # the default metric is the L2 module, counted where it was
    before = losses.native_calls.get('nearest', 0)
    assert torch.equal(losses.StyleLossNearest(target)(x), losses.StyleLossNearest(target, 'l2')(x))
    assert losses.native_calls.get('nearest', 0) == before + 2


def test_the_operators_refuse_what_they_cannot_run():
    from style_transfer import _hip as hip
    lib = hip.load_library()
    x = torch.zeros(1 << 16, device=DEV)
    idx = torch.zeros(64, device=DEV, dtype=torch.int32)
    assert x.data_ptr() % 256 == 0
    px, pi = hip._ptr(x), ctypes.c_void_p(idx.data_ptr())
    off = ctypes.c_void_p(x.data_ptr() + 16)
    too_many = hip.max_pixels() + 1

    def refused(rc, *words):
        assert rc != 0
        message = lib.st_last_error().decode()
        for word in words:
            assert word in message, (word, message)
    for c, n, m, word in ((48, 4, 4, 'multiple of 32'), (64, 0, 4, 'at least one'), (64, 4, 0, 'at least one'),
                          (64, too_many, 4, str(hip.max_pixels())), (64, 4, too_many, str(hip.max_pixels()))):
        refused(lib.st_op_nearest_cosine_loss(px, c, n, px, m, px, pi, px, px, None), word, 'st_op_nearest_cosine_loss')
    refused(lib.st_op_nearest_cosine_prepare(px, 48, 4, 0, px, None), 'multiple of 32', 'st_op_nearest_cosine_prepare')
    refused(lib.st_op_nearest_cosine_prepare(px, 64, too_many, 0, px, None), str(hip.max_pixels()))
    for centered in (2, -1):
        refused(lib.st_op_nearest_cosine_prepare(px, 64, 4, centered, px, None), '0 (cosine) or 1 (centered_cosine)')
    refused(lib.st_op_nearest_cosine_prepare(px, 64, 4, 1, off, None), 'prepared must be 256-byte aligned')
    refused(lib.st_op_nearest_cosine_loss(px, 64, 4, off, 4, px, pi, px, px, None), 'prepared must be 256-byte aligned')
    refused(lib.st_op_nearest_cosine_loss(px, 64, 4, px, 4, off, pi, px, px, None), 'scratch must be 256-byte aligned')
    refused(lib.st_op_nearest_cosine_loss(None, 64, 4, px, 4, px, pi, px, px, None), 'null argument')
    # every other buffer may be merely 4-byte aligned: feat, the indices and the gradient 4 bytes off
    c, n, m = 64, 72, 200               # (n a multiple of 4: the aligned call takes the 16-byte path, this one the scalar path)
    f, s = _gauss(c, n, 7), _gauss(c, m, 8)
    prepared = _prepare(s, 'centered_cosine')
    want = hip.op_nearest_cosine_loss(f.to(DEV), prepared, m)
    store = torch.zeros(c * n + 1, device=DEV)
    store[1:] = f.to(DEV).flatten()
    scratch = torch.empty(lib.st_op_nearest_cosine_scratch_floats(c, n, m), device=DEV)
    out = torch.zeros(c * n + 1, device=DEV)
    idx_store = torch.zeros(n + 1, device=DEV, dtype=torch.int32)
    loss = torch.zeros(2, device=DEV)
    assert scratch.data_ptr() % 256 == 0 and prepared.data_ptr() % 256 == 0
    assert lib.st_op_nearest_cosine_loss(ctypes.c_void_p(store.data_ptr() + 4), c, n, hip._ptr(prepared), m, hip._ptr(scratch),
                                         ctypes.c_void_p(idx_store.data_ptr() + 4), ctypes.c_void_p(out.data_ptr() + 4),
                                         ctypes.c_void_p(loss.data_ptr() + 4), None) == 0, lib.st_last_error().decode()
    torch.cuda.synchronize()
    assert torch.equal(out[1:].view(c, n), want[1]) and torch.equal(idx_store[1:].long(), want[2]) and torch.equal(loss[1], want[0])
    assert out[0] == 0 and idx_store[0] == 0 and loss[0] == 0


# ---- 2. plans -----------------------------------------------------------------------------------------------------------------
L2S = ['l2'] * 5


def _names(near, metric):
    """One metric name per style layer: `metric` on the flagged layers, or the list as it is."""
    return list(metric) if isinstance(metric, (list, tuple)) else [metric if flag else 'l2' for flag in near]


def _plan(size, pooling, precision, content_layers, style_layers, kinds, diag, near, metrics, configure=True, style_size=None, samples=None):
    """A plan in the documented order: layers, kinds, diagonal, nearest, nearest metric, weights, targets."""
    from style_transfer import _hip as hip
    net = hip.Net(T._weights(), pooling, DEV, precision)
    plan = hip.Plan(net, *size)
    if configure:
        plan.set_taps(content_layers, style_layers)
    if kinds is not None:
        plan.set_layer_loss_kinds(*kinds)
    if diag is not None and any(diag):
        plan.set_w2_diagonal(diag)
    plan.set_style_nearest(near)
    assert plan.nearest_metric == ('l2',) * len(style_layers)
    if metrics is not None:
        plan.set_nearest_metric(metrics)
        assert plan.nearest_metric == tuple(metrics) and plan.style_nearest == tuple(bool(v) for v in near)
    plan.set_loss_weights(*T._layer_weights(content_layers, style_layers), T.TV_WEIGHT)
    NG._set_targets(plan, size, pooling, content_layers, style_layers, near, None, style_size, samples)
    return net, plan


def _term(feat, vectors, metric, k):
    """include/st_amd.h's term of a flagged entry before its weight in feat's dtype, the matches k and mu held constant."""
    if metric == 'l2':
        return NG._nearest_term(feat, vectors.to(feat.dtype), k)
    mu, unit = (t.to(feat.dtype) for t in _parts(vectors, metric))
    g = feat[0].flatten(1) - mu[:, None]
    p = (g * unit[:, k]).sum(0)
    return (1 - p / torch.sqrt((g * g).sum(0) + EPS)).mean()


def _own_term(mat64, vectors, metric):
    """The term of `metric` on the float64 tap at that metric's own float64 matches."""
    if metric == 'l2':
        k = NG._distances(mat64.float(), vectors)[1]
    else:
        k = _first_argmax(_scores(mat64, *_parts(vectors, metric)))
    return float(_term(mat64[None], vectors, metric, k))


def _oracle(image, pooling, decisions, content_layers, style_layers, ctargets, moments, sets, matches, weights, kinds, diag, near, metrics,
            clevels, tvmap, lap, dtype, others=False):
    """SumLoss in `dtype`: (weighted content terms, weighted style terms, the image-space term, gradient and - others - per flagged
    layer the weighted terms of all three metrics on the same tap, each at its own float64 matches)."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    cws, sws = weights
    img = image.to(dtype).clone().requires_grad_(True)
    feats = O.vgg_features(img, T._weights() if dtype == torch.float32 else T._weights64(), content_layers + style_layers, pooling,
                           decisions)
    cterms = []
    for layer, cw, kind in zip(content_layers, cws, kinds[0]):
        wmap = None if clevels is None else clevels[MG.LEVEL[layer]].to(dtype)
        cterms.append(CM.weighted_content(feats[layer], ctargets[layer].to(dtype), wmap, kind, 1e-8) * cw)
    sterms = []
    for j, (layer, sw, kind) in enumerate(zip(style_layers, sws, kinds[1])):
        if near[j]:
            sterms.append(_term(feats[layer], sets[j], metrics[j], matches[j]) * sw)
        else:
            sterms.append(D._style_term(feats[layer], layer, moments[layer], None, kind, diag[j], None, dtype) * sw)
    space = (O.tv_loss(img) if tvmap is None else CM.weighted_tv(img, tvmap.to(dtype))) * T.TV_WEIGHT
    if lap is not None:
        for term in formula_terms(img, lap[0].to(dtype), lap[1]):
            space = space + term * lap[2]
    total = sum(cterms) + sum(sterms) + space
    (grad,) = torch.autograd.grad(total, img)
    alt = None
    if others:
        with torch.no_grad():
            alt = [{name: _own_term(feats[layer][0].flatten(1).double(), sets[j], name) * sw for name in ('l2',) + METRICS} if near[j] else None
                   for j, (layer, sw) in enumerate(zip(style_layers, sws))]

    def f(t):
        return float(t.detach())
    return [f(t) for t in cterms], [f(t) for t in sterms], f(space), grad.detach(), alt


def _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, near, metrics, lap_pools=None, style_size=None,
           samples=None):
    """One closure of `plan` against the oracle under the plan's OWN maps and matches; returns the failures."""
    from style_transfer import _hip as hip
    size = tuple(image.shape[2:])
    decisions = L._decisions(plan, img, pooling, content_layers, style_layers)

    def held(read):
        try:
            return read()
        except hip.HipLibraryError:
            return None
    clevels = held(lambda: CM._content_levels(plan))
    tvmap = held(lambda: plan.tv_mask().cpu().double())
    lap = None if lap_pools is None else (LG._content(size), lap_pools, LG.LAP_WEIGHT)
    losses, grad = plan.loss_and_grad(img)
    torch.cuda.synchronize()
    terms = plan.term_losses().cpu().numpy()
    losses = losses.cpu().numpy()
    grad = grad.clone()
    nc, ns = len(content_layers), len(style_layers)
    sets = [NG._style_vectors(size, pooling, layer, style_size, samples) if near[j] else None for j, layer in enumerate(style_layers)]
    matches = [plan.nearest_indices(layer).cpu() if near[j] else None for j, layer in enumerate(style_layers)]
    # the matches on the plan's own tap, read back: the deficit check of the header, every pixel, by the entry's metric
    plan.forward(img, max(content_layers + style_layers))
    for j, layer in enumerate(style_layers):
        if near[j]:
            tap = plan.feature(layer).cpu()[0].flatten(1)
            assert matches[j].shape == (tap.shape[1],)
            what = f'{tag} style[{layer}] {tap.shape[1]} pixels against {sets[j].shape[1]} vectors'
            if metrics[j] == 'l2':
                NG._check_deficit(what, tap, sets[j], matches[j])
            else:
                _check_deficit(what, tap, sets[j], metrics[j], matches[j])
    ctargets, moments = T._targets(size, pooling, content_layers, style_layers)
    args = (image, pooling, decisions, content_layers, style_layers, ctargets, moments, sets, matches,
            T._layer_weights(content_layers, style_layers), kinds, diag, near, metrics, clevels, tvmap, lap)
    c32, s32, sp32, g32, _ = _oracle(*args, torch.float32)
    c64, s64, sp64, g64, alt = _oracle(*args, torch.float64, others=True)
    assert len(terms) == nc + ns + 1 and np.isfinite(terms).all() and np.isfinite(losses).all(), f'{tag}: terms {terms}'
    failures = []

    def check(name, got, want32, want64):
        floor = abs(want32 - want64) / abs(want64)
        tol = max(T.TERM_TOL, 3 * floor)
        rel = abs(got - want32) / abs(want32)
        print(f'[nearest-cosine] {tag} term {name:24s} got {got:.8g} want {want32:.8g} rel {rel:.2e}  floor {floor:.2e}  bar {tol:.1e}  '
              f'{"PASS" if rel <= tol else "FAIL"}')
        if not rel <= tol:
            failures.append(f'{tag}: term {name} rel {rel:.2e} > {tol:.1e}')
    for i, layer in enumerate(content_layers):
        check(f'content[{layer}]', float(terms[i]), c32[i], c64[i])
    for j, layer in enumerate(style_layers):
        if not near[j]:
            check(f'style[{layer}] {"diagonal w2" if diag[j] else kinds[1][j]}', float(terms[nc + j]), s32[j], s64[j])
            continue
        rel = abs(float(terms[nc + j]) - s64[j]) / abs(s64[j])
        print(f'[nearest-cosine] {tag} term style[{layer}] {metrics[j]:16s} got {float(terms[nc + j]):.8g} float64 {s64[j]:.8g} rel {rel:.2e}  '
              f'bar {BAR:.0e}  {"PASS" if rel <= BAR else "FAIL"}')
        if not rel <= BAR:
            failures.append(f'{tag}: term style[{layer}] {metrics[j]} rel {rel:.2e} > {BAR:.0e}')
        # an ignored or mixed-up metric cannot pass: the other two metrics' terms of the same tap are far from this one
        for name, value in alt[j].items():
            if name == metrics[j]:
                continue
            ratio = abs(value - s64[j]) / abs(s64[j]) / BAR
            print(f'[nearest-cosine] {tag} style[{layer}]: the {name} term {value:.6g} is {ratio:.0f} bars from the {metrics[j]} one {s64[j]:.6g}')
            assert ratio >= IGNORED_BARS, f'{tag}: style[{layer}]: the {name} term is {ratio:.1f} bars away only'
    check('image-space (tv, laplacian)', float(terms[-1]), sp32, sp64)
    want_total = np.float32(0)
    for t in terms.astype(np.float32):
        want_total = np.float32(want_total + t)
    rel_total = abs(float(losses[7]) - float(want_total)) / abs(float(want_total))
    if not rel_total <= T.SUM_TOL:
        failures.append(f'{tag}: total rel {rel_total:.2e} > {T.SUM_TOL:.0e}')
    assert torch.isfinite(grad).all(), f'{tag}: non-finite gradient'
    err, floor = rel_l2(grad.cpu(), g64), rel_l2(g32, g64)
    print(f'[nearest-cosine] {tag} gradient hip-vs-fp64 {err:.2e}  ref-fp32 floor {floor:.2e}  bar {BAR:.0e}  {"PASS" if err <= BAR else "FAIL"}')
    if not err <= BAR:
        failures.append(f'{tag}: gradient rel-L2 {err:.2e} > {BAR:.0e} (fp32 composition: {floor:.2e})')
    return failures


MIXED = ['l2', 'l2', 'l2', 'cosine', 'centered_cosine']
CASES = [
    # name, size, pooling, precision, (content layers, style layers), style kinds, diagonal, nearest, metric(s), configure, style size, samples
    ('all-five-cosine', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, ALL, 'cosine', False, None, None),
    ('all-five-centered-odd-fp32', ODD, 'max', 'fp32', T.DEFAULT, W2, NONE, ALL, 'centered_cosine', False, None, None),
    ('all-five-centered-average', SIZE, 'average', 'fp16x3', T.DEFAULT, W2, NONE, ALL, 'centered_cosine', False, None, None),
    ('all-five-cosine-style-56x44', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, ALL, 'cosine', False, (56, 44), None),
    ('all-five-centered-400-samples', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, ALL, 'centered_cosine', False, None, 400),
    ('deep-two-cosine-odd', ODD, 'max', 'fp16x3', T.DEFAULT, W2, NONE, DEEP, 'cosine', False, None, None),
    ('deep-two-centered-fp32-average', SIZE, 'average', 'fp32', T.DEFAULT, W2, NONE, DEEP, 'centered_cosine', False, None, None),
    ('mixed-l2-cosine-centered', SIZE, 'max', 'fp16x3', T.DEFAULT, W2, NONE, [True, False, False, True, True], MIXED, False, None, None),
    ('beside-gram-and-diagonal', SIZE, 'max', 'fp16x3', T.DEFAULT, ['w2', 'gram', 'w2', 'w2', 'w2'], [True, False, False, False, False],
     DEEP, ['l2', 'l2', 'l2', 'centered_cosine', 'cosine'], False, None, None),
    ('a-layer-in-both-lists', SIZE, 'max', 'fp16x3', T.CONFIGS['b'], W2, NONE, DEEP, 'centered_cosine', True, None, None),
]


@pytest.mark.parametrize('name, size, pooling, precision, lists, style_kinds, diag, near, metric, configure, style_size, samples', CASES,
                         ids=[c[0] for c in CASES])
def test_configurations(name, size, pooling, precision, lists, style_kinds, diag, near, metric, configure, style_size, samples):
    content_layers, style_layers = lists
    kinds = (['mse'] * len(content_layers), style_kinds)
    metrics = _names(near, metric)
    image = T._inputs(size, pooling)['image']
    img = image.to(DEV)
    _, plan = _plan(size, pooling, precision, content_layers, style_layers, None if style_kinds == W2[:len(style_kinds)] else kinds,
                    diag, near, metrics, configure, style_size, samples)
    tag = f'({name}) style {style_layers} metrics {metrics} {size[0]}x{size[1]}-{pooling}-{precision}'
    failures = _judge(tag, plan, img, image, pooling, content_layers, style_layers, kinds, diag, near, metrics, style_size=style_size,
                      samples=samples)
    assert not failures, '; '.join(failures)


def test_both_maps_and_the_laplacian():
    near = [True, False, True, False, True]
    metrics = ['cosine', 'l2', 'centered_cosine', 'l2', 'centered_cosine']
    image = T._inputs(SIZE, 'max')['image']
    _, plan = _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, near, metrics, configure=False)
    plan.set_content_mask(MG.ramp_mask(*SIZE).to(DEV))
    plan.set_tv_mask(MG.binary_mask(*SIZE).to(DEV))
    plan.set_laplacian(LG._content(SIZE).to(DEV), (4, 16), LG.LAP_WEIGHT)
    failures = _judge('content map + TV map + Laplacian', plan, image.to(DEV), image, 'max', *T.DEFAULT, (MSE, W2), NONE, near, metrics,
                      lap_pools=(4, 16))
    assert not failures, '; '.join(failures)


# ---- 3. bits and steps --------------------------------------------------------------------------------------------------------
def _flagged_plan(near=(True, False, False, True, True), metrics=('cosine', 'l2', 'l2', 'centered_cosine', 'cosine')):
    return _plan(SIZE, 'max', 'fp16x3', *T.DEFAULT, None, None, list(near), None if metrics is None else list(metrics), configure=False)[1]


def test_two_closures_are_equal_steps_are_closure_plus_update_and_the_range_guard_runs():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    plan = _flagged_plan()
    first = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()] + [plan.nearest_indices(layer) for layer in (1, 20, 29)]
    second = [t.clone() for t in plan.loss_and_grad(img)] + [plan.term_losses().clone()] + [plan.nearest_indices(layer) for layer in (1, 20, 29)]
    torch.cuda.synchronize()
    assert T._same(first, second) and all(torch.isfinite(t).all() for t in first[:3])
    xa, ma, va, ea = T._state(img)
    xb, mb, vb, eb = T._state(img)
    for k in (1, 2, 3):
        la = plan.step(xa, ma, va, ea, k, 0.02).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        plan.apply_update(xb, g, mb, vb, eb, k, 0.02)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (k, la, lb)
        assert torch.equal(xa, xb) and torch.equal(ma, mb) and torch.equal(va, vb) and torch.equal(ea, eb), k
    assert not torch.equal(xa, img)
    # the native L-BFGS step
    xa, _, _, ea = T._state(img)
    xb, _, _, eb = T._state(img)
    opt_a, opt_b = hip.LBFGS(xa), hip.LBFGS(xb)
    for k in (1, 2, 3):
        la = opt_a.step(plan, xa, ea, 0.99).clone()
        lb, g = plan.loss_and_grad(xb)
        lb = lb.clone()
        opt_b.update(xb, g, eb, 0.99)
        torch.cuda.synchronize()
        assert torch.equal(la, lb), (k, la, lb)
        assert torch.equal(xa, xb) and torch.equal(ea, eb), k
    assert opt_a.info() == opt_b.info() and not torch.equal(xa, img)
    before = K._leg(plan, img, steps=False)
    fwd, bwd = plan.range_guard(img)
    assert not any(fwd) and not any(bwd)
    assert T._same(before, K._leg(plan, img, steps=False))


def test_metrics_all_l2_and_set_then_cleared_are_the_untouched_flagged_plan():
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    near = [True, False, False, True, True]
    want = K._leg(NG._flagged_plan(near), img, steps=True)
    assert T._same(want, K._leg(_flagged_plan(near, L2S), img, steps=True))
    cleared = _flagged_plan(near)
    assert not torch.equal(K._leg(cleared, img, steps=False)[0], want[0])
    cleared.set_nearest_metric(None)
    assert cleared.nearest_metric == ('l2',) * 5 and cleared.style_nearest == tuple(near)
    NG._set_targets(cleared, SIZE, 'max', *T.DEFAULT, near)
    assert T._same(want, K._leg(cleared, img, steps=True))
    # set_style_nearest itself resets every metric
    again = _flagged_plan(near)
    again.set_style_nearest(near)
    assert again.nearest_metric == ('l2',) * 5
    NG._set_targets(again, SIZE, 'max', *T.DEFAULT, near)
    assert T._same(want, K._leg(again, img, steps=True))


def test_cosine_is_centered_cosine_in_bits_when_the_style_mean_is_zero():
    """A symmetric set {s, -s} has the mean exactly 0 (the double sum in ascending k cancels pair by pair when the copies
    alternate), so mu = 0, b = 0 and the two metrics prepare the same rows: this pins the bias path."""
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    legs = []
    for metric in METRICS:
        plan = _flagged_plan(DEEP, None)
        plan.set_nearest_metric(metric)
        NG._set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
        for j, layer in ((3, 20), (4, 29)):
            half = NG._style_vectors(SIZE, 'max', layer)
            both = torch.stack([half, -half], dim=2).flatten(1).contiguous()           # s_0, -s_0, s_1, -s_1, ...
            plan.set_style_vectors(j, both.to(DEV))
        legs.append(K._leg(plan, img, steps=False) + [plan.nearest_indices(20), plan.nearest_indices(29)])
    assert T._same(legs[0], legs[1])
    # ... and with the real, non-zero mean the two differ
    assert not torch.equal(K._leg(_flagged_plan(DEEP, _names(DEEP, 'cosine')), img, steps=False)[0],
                           K._leg(_flagged_plan(DEEP, _names(DEEP, 'centered_cosine')), img, steps=False)[0])


# ---- 4. setter semantics ------------------------------------------------------------------------------------------------------
def test_setter_semantics():
    from style_transfer import _hip as hip
    img = T._inputs(SIZE, 'max')['image'].to(DEV)
    net = hip.Net(T._weights(), 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, *SIZE)
    lib = plan.lib
    ints = NG._ints

    def refused(call, *words):
        assert call() != 0
        message = lib.st_last_error().decode()
        for word in words:
            assert word in message, (word, message)
    assert plan.nearest_metric == ('l2',) * 5
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    before = K._leg(plan, img, steps=False)
    # refusals carry a message and leave the plan as it was, targets included
    refused(lambda: lib.st_plan_set_nearest_metric(plan.handle, ints(0, 0, 0, 0, 1)), 'not flagged', 'st_plan_set_nearest_metric')
    refused(lambda: lib.st_plan_set_nearest_metric(plan.handle, ints(0, 0, 0, 0, 3)), '0 (l2), 1 (cosine) or 2 (centered_cosine)')
    refused(lambda: lib.st_plan_set_nearest_metric(plan.handle, ints(-1, 0, 0, 0, 0)), '0 (l2)')
    refused(lambda: lib.st_plan_set_nearest_metric(None, ints(0, 0, 0, 0, 0)), 'null plan')
    refused(lambda: lib.st_plan_nearest_metric(plan.handle, None), 'null argument')
    assert T._same(before, K._leg(plan, img, steps=False))
    with pytest.raises(ValueError, match='one per layer'):
        plan.set_nearest_metric(['cosine'] * 4)
    with pytest.raises(ValueError, match='nearest metric'):
        plan.set_nearest_metric(['l2', 'l2', 'l2', 'l2', 'chebyshev'])
    # a successful call - all zeros or null included - drops every target, like the other option setters
    assert lib.st_plan_set_nearest_metric(plan.handle, None) == 0
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    assert T._same(before, K._leg(plan, img, steps=False))
    # the order of configuration: nearest, then the metric; a name alone goes to the flagged layers
    plan.set_style_nearest(DEEP)
    refused(lambda: lib.st_plan_set_nearest_metric(plan.handle, ints(2, 0, 0, 2, 2)), 'style layer 0 is not flagged')
    assert plan.nearest_metric == ('l2',) * 5
    plan.set_nearest_metric('centered_cosine')
    assert plan.nearest_metric == ('l2', 'l2', 'l2', 'centered_cosine', 'centered_cosine')
    plan.set_nearest_metric(['l2', 'l2', 'l2', 'cosine', 'l2'])
    assert plan.nearest_metric == ('l2', 'l2', 'l2', 'cosine', 'l2')
    # a custom eps is refused on a flagged entry whatever its metric, as before
    refused(lambda: lib.st_plan_set_loss_eps(plan.handle, None, (ctypes.c_float * 5)(-1, -1, -1, 1e-3, -1)), 'nearest')
    # the targets: dropped by the setter; the set is prepared by the entry's metric and its buffers sized by it
    NG._set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
    assert torch.isfinite(plan.loss_and_grad(img)[0]).all()
    plan.set_nearest_metric('cosine')
    with pytest.raises(hip.HipLibraryError, match=r'content target 0 \(features\[22\]\)'):
        plan.loss_and_grad(img)
    NG._set_targets(plan, SIZE, 'max', *T.DEFAULT, DEEP)
    first = plan.loss_and_grad(img)[0].clone()
    vectors = NG._style_vectors(SIZE, 'max', 29)
    k = plan.nearest_indices(29)
    assert k.shape == (6,) and k.dtype == torch.int64 and int(k.min()) >= 0 and int(k.max()) < vectors.shape[1]
    # a larger and then a smaller style set on the same entry
    bigger = torch.cat([vectors, vectors.flip(1) * 0.5, vectors * 2.0 + 0.1], dim=1).contiguous()
    plan.set_style_vectors(4, bigger.to(DEV))
    plan.loss_and_grad(img)
    tap = plan.feature(29).cpu()[0].flatten(1)
    _check_deficit('a larger style set', tap, bigger, 'cosine', plan.nearest_indices(29).cpu())
    plan.set_style_vectors(4, vectors[:, :5].contiguous().to(DEV))
    plan.loss_and_grad(img)
    _check_deficit('a smaller style set', tap, vectors[:, :5].contiguous(), 'cosine', plan.nearest_indices(29).cpu())
    grown = plan.device_bytes()
    plan.set_style_vectors(4, vectors.to(DEV))
    assert plan.device_bytes() == grown                      # (a smaller set allocates nothing)
    assert torch.equal(plan.loss_and_grad(img)[0], first)
    # either kinds setter, set_taps and set_style_nearest clear the metrics, as they clear the flags
    for clear in (lambda: plan.set_loss_kinds('mse', 'w2'), lambda: plan.set_layer_loss_kinds(MSE, W2), lambda: plan.set_taps(*T.CONFIGS['b']),
                  lambda: plan.set_taps(*T.DEFAULT), lambda: plan.set_style_nearest(DEEP)):
        plan.set_style_nearest(DEEP)
        plan.set_nearest_metric('centered_cosine')
        assert plan.nearest_metric[4] == 'centered_cosine'
        clear()
        assert plan.nearest_metric == ('l2',) * 5
    # back on the default configuration: the fast closure again, equal to a plan that never left it
    plan.set_style_nearest(None)
    T._set_targets(plan, SIZE, 'max', *T.DEFAULT)
    assert T._same(before, K._leg(plan, img, steps=False))


# ---- 5. stylize() -------------------------------------------------------------------------------------------------------------
def test_stylize_reads_style_nearest_metric():
    from style_transfer import StyleTransfer
    st = StyleTransfer(devices=[DEV], pooling='max', weights='synthetic')
    assert st.style_nearest_metric == 'l2'
    content_image, style_images = T._pil(81, 64, 48), [T._pil(82, 60, 44), T._pil(83, 52, 40)]
    seen = []

    def callback(it):
        if it.i == 1:
            seen.append((it.w, it.h, it.loss))

    def run(min_scale=64):
        del seen[:]
        out = st.stylize(content_image, style_images, style_weights=[0.75, 0.25], end_scale=64, min_scale=min_scale, initial_iterations=4,
                         iterations=4, callback=callback)
        assert out is not None and torch.isfinite(st.get_image_tensor()).all()
        return list(seen)

    st.style_nearest, st.style_nearest_samples = DEEP, 10
    l2_loss = run()[0][2]
    assert st._plan.nearest_metric == ('l2',) * 5
    st.style_nearest_metric = 'centered_cosine'
    scales = run(min_scale=45)                       # two scales: the metric is set per scale, after the flags and before the targets
    assert len(scales) == 2 and scales[0][:2] != scales[1][:2]
    assert st._plan.style_nearest == tuple(DEEP) and st._plan.nearest_metric == ('l2', 'l2', 'l2', 'centered_cosine', 'centered_cosine')
    assert scales[1][2] != l2_loss
    # the final closure: finite terms, and matches into the union of the two images' ten sampled vectors each
    final = st.image.detach().clone()
    st._plan.loss_and_grad(final)
    torch.cuda.synchronize()
    got = st._plan.term_losses().cpu().numpy()
    st._plan.forward(final, 29)
    for j, layer in ((3, 20), (4, 29)):
        tap = st._plan.feature(layer).cpu()
        k = st._plan.nearest_indices(layer).cpu()
        assert k.shape == (tap[0].flatten(1).shape[1],) and int(k.max()) < 20
    st.style_nearest_metric = ['l2', 'l2', 'l2', 'cosine', 'l2']
    run()
    assert st._plan.nearest_metric == ('l2', 'l2', 'l2', 'cosine', 'l2') and len(got) == 7 and np.isfinite(got).all()
    del st.style_nearest_metric
    assert run()[0][2] == l2_loss and st._plan.nearest_metric == ('l2',) * 5
    # refusals name the attribute and come before any device work
    for bad in ('manhattan', ['cosine'] * 5, ['l2'] * 4):
        st.style_nearest_metric = bad
        with pytest.raises(ValueError, match='style_nearest_metric'):
            st.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    two = StyleTransfer(devices=[DEV, DEV], pooling='max', weights='synthetic')
    two.style_nearest, two.style_nearest_metric = DEEP, 'cosine'
    before = torch.cuda.memory_allocated()
    with pytest.raises(ValueError, match='style_nearest.* on 2 ranks'):
        two.stylize(content_image, style_images[:1], end_scale=64, min_scale=64, initial_iterations=1, iterations=1)
    assert torch.cuda.memory_allocated() == before


# ---- 6. caller-owned buffers --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n, m', [(1, 1), (127, 127), (132, 513), (256, 1025)])
def test_the_entries_stay_inside_fenced_buffers_of_the_promised_sizes(n, m):
    """tests/test_caller_buffers_gpu.py's harness on the cosine entries: every buffer fenced and poisoned, `prepared` and `scratch`
    of exactly the promised sizes and pre-filled with 0xFF, inputs and outputs shifted off 16-byte alignment - the fences stay
    intact, every output element is written, two calls and every shift give the same bits."""
    import test_caller_buffers_gpu as CB
    lib, c = CB._lib(), 64
    f, s = _gauss(c, n, 3100 + n), _gauss(c, m, 4100 + m)
    for metric in METRICS:
        base = None
        for si, so in (CB.SHIFTS if n % 4 == 0 else CB.RAGGED_SHIFTS):
            tag = f'nearest cosine ({c}, {n}, {m}) {metric} shift {(si, so)}'
            b = CB.Buffers()
            feat, vectors = b.inp('feat', f, si), b.inp('vectors', s, si)
            up = b.inp('upstream', torch.tensor([CB.UPSTREAM]), so)
            prepared = b.scratch('prepared', 4 * int(lib.st_op_nearest_cosine_prepared_floats(c, m)), 256)
            scratch = b.scratch('scratch', 4 * int(lib.st_op_nearest_cosine_scratch_floats(c, n, m)), 256)
            idx, unit, loss, grad = b.out('idx', n, so, torch.int32), b.out('unit', c * n, so), b.out('loss', 1, so), b.out('grad', c * n, so)

            def call():
                CB._ok(lib.st_op_nearest_cosine_prepare(vectors, c, m, int(metric == 'centered_cosine'), prepared, CB._stream()), tag)
                CB._ok(lib.st_op_nearest_cosine_loss(feat, c, n, prepared, m, scratch, idx, unit, loss, CB._stream()), tag)
                CB._ok(lib.st_op_nearest_loss_backward(unit, c * n, up, grad, CB._stream()), tag)
            call()
            b.verify(tag)
            first = b.bits()
            call()
            b.verify(tag)
            CB._same_bits(tag, first, b.bits())
            got = {name: b.get(name) for name in first}
            k = got['idx'].to(torch.int64)
            _check_deficit(tag, f, s, metric, k)
            want, want_grad = _formula(f, s, metric, k)
            assert abs(float(got['loss'][0]) - want) <= BAR * abs(want)
            if float(want_grad.norm()):
                assert rel_l2(got['grad'].double().reshape(c, n), CB.UPSTREAM * want_grad) <= BAR
            base = base or got
            for name in ('idx', 'unit', 'loss', 'grad'):                       # the 16-byte and the scalar path: the same bits
                assert torch.equal(got[name], base[name]), (tag, name)
