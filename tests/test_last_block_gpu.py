"""The kernels that finish a sum in their last workgroup (content MSE, scaled-MSE sums, TV border, Laplacian, channel
statistics, marginal and nearest residuals; csrc/st_common.h LastBlock) hand their per-workgroup partial sums over WRITE-THROUGH:
thread 0 stores them with agent-scope relaxed atomic stores, waits for them and takes the ticket - no release fence.
ST_LAST_BLOCK_FENCE=1 selects the former hand-off (plain stores behind an agent-scope release fence).  Grid, partial layout and
the order of the last workgroup's sum are the same, so every value must keep its bits; and a launch whose last workgroup read a
partial before it was visible - a stale one of the launch before, on the same ticket and buffer - would show as a loss that
differs from the one the same input gives on an idle device (profiles/last_block.md).

Tolerances against float64 are the existing ones: the MSE value and gradient 1e-4 (tests/test_native_losses_gpu.py TERM_TOL and
bar() at that file's floor), the TV value and gradient 2e-6 (tests/test_kernels_gpu.py test_tv_loss_and_gradient), a term of the
closure 1e-4 (tests/test_hot_path_gpu.py TERM_TOL)."""
import pytest
import torch

import st_oracle as O
import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TERM_TOL = 1e-4
TV_TOL = 2e-6

# content MSE, 16-byte groups of four floats, 256 per workgroup, at most 2048 workgroups: 1, 33 and 2048 of them (2^21 floats
# is relu4_2 at 512^2) - and 1 and 33 on the one-float-at-a-time path (count % 4 != 0)
MSE_COUNTS = [(1000, 1), (4 * (32 * 256 + 5), 33), (1 << 21, 2048), (250, 1), (32 * 256 + 5, 33)]
# TV: (H, W, workgroups of the border launch, which holds the last one).  W % 4 != 0: the border kernel walks all 3 H W pixels,
# 256 per workgroup, at most 2048; else it walks the border groups after the interior launch has left its partials
TV_SHAPES = [(5, 13, 1), (216, 13, 33), (419, 419, 2048), (64, 512, 18), (128, 128, 7)]


def _hip():
    from style_transfer import _hip as hip
    return hip


def _pair(count, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(count, generator=g, device=DEV).relu_()
    t = torch.randn(count, generator=g, device=DEV).relu_()
    return x, t


def _image(h, w, seed):
    return synth.smooth_image(seed, max(h, 16), max(w, 16))[..., :h, :w].contiguous().to(DEV)


def _both(fn):
    """fn() under the write-through hand-off, under the release fence, and under the write-through one again."""
    hip, out = _hip(), []
    for fence in (0, 1, 0):
        with hip.options(ST_LAST_BLOCK_FENCE=fence):
            out.append(fn())
        torch.cuda.synchronize()
    return out


def _assert_equal(tag, runs):
    new, old, again = runs
    for k, other in (('fence', old), ('repeat', again)):
        assert len(new) == len(other)
        for i, (a, b) in enumerate(zip(new, other)):
            assert torch.equal(a, b), (tag, k, i, float((a - b).abs().max()))


@pytest.mark.parametrize('count,blocks', MSE_COUNTS, ids=lambda v: str(v))
def test_mse_term_has_the_same_bits_under_both_hand_offs_and_meets_float64(count, blocks):
    hip = _hip()
    x, t = _pair(count, 100 + blocks + count % 7)
    weight = 0.015
    new = _both(lambda: hip.op_mse_term(x, t, weight))
    _assert_equal(f'mse {count}', new)
    loss, grad = new[0]
    d = x.double() - t.double()
    want = weight * float(d.square().mean())
    want_g = d * (2 * weight / count)
    rel = abs(float(loss) - want) / want
    err = float((grad.double() - want_g).norm() / want_g.norm())
    print(f'[last-block] mse term, {count} floats in {blocks} workgroup(s): both hand-offs bit-identical; value rel={rel:.3e} '
          f'(tol {TERM_TOL:.1e}), gradient rel_l2={err:.3e} (tol {TERM_TOL:.1e})')
    assert rel <= TERM_TOL and err <= TERM_TOL


@pytest.mark.parametrize('h,w,blocks', TV_SHAPES, ids=lambda v: str(v))
def test_tv_term_has_the_same_bits_under_both_hand_offs_and_meets_float64(h, w, blocks):
    hip = _hip()
    img = _image(h, w, 40 + blocks)
    weight = 2.0
    new = _both(lambda: hip.op_tv_term(img, weight))
    _assert_equal(f'tv {h}x{w}', new)
    loss, grad = new[0]
    want, want_g = O.tv_loss_grad_closed_form(img.double())
    rel = abs(float(loss) - weight * float(want)) / (weight * float(want))
    err = float((grad.double() - weight * want_g).norm() / (weight * want_g).norm())
    print(f'[last-block] tv term {h}x{w}, {blocks} border workgroup(s): both hand-offs bit-identical; value rel={rel:.3e} '
          f'(tol {TV_TOL:.1e}), gradient rel_l2={err:.3e} (tol {TV_TOL:.1e})')
    assert rel < TV_TOL and err <= TV_TOL


def _plan(hip, weights, content, style, size):
    net = hip.Net(weights, 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, size, size)
    plan.forward(content, 22)
    plan.set_content_target_from_forward()
    content_feat = plan.feature(22).clone()
    plan.forward(style, 29)
    for i, layer in enumerate(O.STYLE_LAYERS):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, O.STYLE_LAYER_WEIGHTS, 2.0)
    return net, plan, content_feat


def test_closure_and_step_have_the_same_bits_under_both_hand_offs(vgg_weights):
    """128^2, the shipped arithmetic: 5 closures and 6 fused iterations on a plan created under each hand-off (a captured closure
    keeps the flavour it was captured with).  The eight losses, the gradient, the image, the EMA and both Adam moments are compared
    with torch.equal; the two terms whose sums the last workgroup finishes - content and TV - are held against float64 on the
    plan's own relu4_2 features and on the image."""
    hip = _hip()
    size = 128
    content, style, image0 = (synth.smooth_image(seed, size, size).to(DEV) for seed in (3, 4, 5))
    keep = {}

    def run():
        out = []
        net, plan, content_feat = _plan(hip, vgg_weights, content, style, size)
        image = image0.clone()
        for _ in range(5):
            l, g = plan.loss_and_grad(image)
            out += [l.clone(), g.clone()]
        plan.forward(image, 22)
        keep['feat'], keep['target'] = plan.feature(22).clone(), content_feat
        m, v, ema = torch.zeros_like(image), torch.zeros_like(image), 0.01 * image
        for step in range(1, 7):
            losses = plan.step(image, m, v, ema, step, 0.02)
            out += [losses.clone(), image.clone(), ema.clone(), m.clone(), v.clone()]
        torch.cuda.synchronize()
        return out

    runs = _both(run)
    assert len(runs[0]) == 5 * 2 + 6 * 5
    _assert_equal('plan 128', runs)
    for k in range(1, 5):                                           # a closure and its own repeats
        assert torch.equal(runs[0][0], runs[0][2 * k]) and torch.equal(runs[0][1], runs[0][2 * k + 1]), k
    losses = runs[0][0].double().cpu()
    assert losses.numel() == 8
    want_content = 0.015 * float((keep['feat'].double() - keep['target'].double()).square().mean())
    want_tv = 2.0 * float(O.tv_loss(image0.double()))
    rel_c = abs(float(losses[0]) - want_content) / want_content
    rel_tv = abs(float(losses[6]) - want_tv) / want_tv
    total = float(losses[7])
    print(f'[last-block] 128^2: 5 closures and 6 iterations bit-identical under both hand-offs; content term rel={rel_c:.3e}, '
          f'TV term rel={rel_tv:.3e} against float64 (tol {TERM_TOL:.1e}); loss {total:.6f}')
    assert rel_c <= TERM_TOL and rel_tv <= TERM_TOL
    assert total > 0 and abs(total - float(losses[:7].sum())) <= 1e-6 * abs(total)


def _busy(side, buf, launches):
    """`launches` passes of buf += 1 (256 MB read and written each) on the side stream."""
    with torch.cuda.stream(side):
        for _ in range(launches):
            buf.add_(1.0)


@pytest.mark.parametrize('fence', [0, 1], ids=['write-through', 'release-fence'])
def test_back_to_back_mse_launches_beside_a_bandwidth_hog_never_read_a_stale_partial(fence):
    """200 launches of the 2048-workgroup content MSE back to back on ONE ticket and partial buffer, the input alternating between
    two tensors whose partial sums differ in every workgroup, while a second stream streams 256 MB through add_ over and over.  The
    last workgroup of a launch finds the previous launch's partials in its XCD's L2 (the previous last workgroup read all of them):
    every loss must have the bits its input gave on an idle device."""
    hip = _hip()
    count, launches = 1 << 21, 200
    xa, t = _pair(count, 7)
    xb = (_pair(count, 8)[0] * 1.5).contiguous()
    with hip.options(ST_LAST_BLOCK_FENCE=fence):
        scratch = hip.term_scratch(DEV)
        idle, parts = [], []
        for x in (xa, xb):
            loss, _ = hip.op_mse_term(x, t, 1.0, scratch=scratch)
            torch.cuda.synchronize()
            idle.append(loss.clone())
            parts.append(scratch[0][:2048].clone())
        assert bool((parts[0] != parts[1]).all()), 'the two inputs must differ in every workgroup\'s partial sum'
        assert not torch.equal(idle[0], idle[1])
        losses = torch.zeros(launches, device=DEV)
        grad = torch.empty_like(xa)
        hog = torch.zeros(64 << 20, device=DEV)                     # 256 MB
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        _busy(side, hog, 20)                                        # running before the first launch
        for i in range(launches):
            hip.op_mse_term(xb if i & 1 else xa, t, 1.0, scratch=scratch, loss=losses[i:i + 1], grad=grad)
            if i % 4 == 0:
                _busy(side, hog, 2)
        torch.cuda.synchronize()
    want = torch.stack([idle[i & 1][0] for i in range(launches)])
    bad = (losses != want).nonzero().flatten().tolist()
    print(f'[last-block] {launches} back-to-back 2048-workgroup MSE launches beside a 256 MB add_ loop ({"release fence" if fence else "write-through"}): '
          f'{len(bad)} differ from the idle device\'s bits; losses {float(idle[0]):.8g} / {float(idle[1]):.8g}')
    assert not bad, (bad[:10], losses[bad[:10]].tolist())
    assert int(scratch[1][0]) == 0, 'the ticket word must be left zero'


@pytest.mark.parametrize('fence', [0, 1], ids=['write-through', 'release-fence'])
def test_back_to_back_tv_launches_beside_a_bandwidth_hog_never_read_a_stale_partial(fence):
    """The same for the TV term on a 64 x 512 image: 96 interior workgroups' partials from the launch before, 18 border workgroups
    and the ticket, 200 times on one scratch, two images in turn."""
    hip = _hip()
    launches = 200
    ia, ib = _image(64, 512, 21), (_image(64, 512, 22) * 0.7).contiguous()
    with hip.options(ST_LAST_BLOCK_FENCE=fence):
        scratch = hip.term_scratch(DEV)
        idle, parts = [], []
        for img in (ia, ib):
            loss, _ = hip.op_tv_term(img, 2.0, scratch=scratch)
            torch.cuda.synchronize()
            idle.append(loss.clone())
            parts.append(scratch[0][:4 * (96 + 18)].clone())
        differ = (parts[0] != parts[1]).view(-1, 4).any(dim=1)      # (a workgroup's four sums; one of them may be 0 in both)
        assert bool(differ.all()), 'the two images must differ in every workgroup\'s partial sums'
        losses = torch.zeros(launches, device=DEV)
        grad = torch.empty_like(ia)
        hog = torch.zeros(64 << 20, device=DEV)
        side = torch.cuda.Stream(device=DEV)
        torch.cuda.synchronize()
        _busy(side, hog, 20)
        for i in range(launches):
            hip.op_tv_term(ib if i & 1 else ia, 2.0, scratch=scratch, loss=losses[i:i + 1], grad=grad)
            if i % 8 == 0:
                _busy(side, hog, 2)
        torch.cuda.synchronize()
    want = torch.stack([idle[i & 1][0] for i in range(launches)])
    bad = (losses != want).nonzero().flatten().tolist()
    print(f'[last-block] {launches} back-to-back TV launches (64 x 512) beside a 256 MB add_ loop ({"release fence" if fence else "write-through"}): '
          f'{len(bad)} differ from the idle device\'s bits')
    assert not bad, (bad[:10], losses[bad[:10]].tolist())
    assert int(scratch[1][0]) == 0, 'the ticket word must be left zero'
