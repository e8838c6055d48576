"""The native ``optimizer='lbfgs'`` step (csrc/st_lbfgs.hip; st_lbfgs_* / st_plan_lbfgs_step in include/st_amd.h) on a
real MI355X: ``torch.optim.LBFGS(max_iter=1, history_size=10)`` in the vector-free form - three launches, every decision of
``LBFGS.step`` a device flag - against torch's own optimiser.

Tolerances and where they come from:
  * stylize(): the bars of tests/test_hot_path_gpu.py for the same fixture (read from the fixture);
  * the recursion against float64: the native run may be no further from ``torch.optim.LBFGS`` in float64 than
    2 x what ``torch.optim.LBFGS`` in fp32 is (the larger of its 1-thread and 8-thread runs: both are fp32 roundings of a
    recursion that amplifies them, and two roundings of it differ by about as much as each does from float64), plus a
    floor of sqrt(n) 2^-24 - the rounding of ONE fp32 evaluation of a sum of n terms - for iterations where both sit at
    rounding level;
  * corner cases: exact statements (bits, counters, flags); iterates to a few ulp of fp32 where one ``axpy`` differs in its
    rounding only;
  * a real size: the 5e-2 relative that tests/test_stylize_sharded_gpu.py applies to two summation orders of this
    recursion; the EMA to 1 ulp of fp32 (the same two fp32 operations).
"""
import numpy as np
import pytest
import torch

from conftest import load_golden
import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP = 2.0 ** -23


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ---- 1. stylize() no longer touches torch.optim.LBFGS ----------------------------------------------------------------
def test_stylize_lbfgs_runs_without_torch_optim(vgg_weights, monkeypatch):
    """stylize(optimizer='lbfgs') is the library's own step: with torch.optim.LBFGS made to raise it completes and meets
    the bars of test_stylize_lbfgs_against_reference (per-sample max(5e-4, 5 x trace_spread), result
    max(1e-4, 5 x result_spread), both from the fixture)."""
    from PIL import Image
    import style_transfer as st_pkg

    def refuse(*a, **k):
        raise AssertionError('torch.optim.LBFGS was constructed: the iteration left the library')
    monkeypatch.setattr(torch.optim, 'LBFGS', refuse)
    g = load_golden('stylize_lbfgs')
    content = Image.fromarray(g['content_u8'], 'RGB')
    styles = [Image.fromarray(g['style0_u8'], 'RGB'), Image.fromarray(g['style1_u8'], 'RGB')]
    st = st_pkg.StyleTransfer(devices=[DEV], weights=vgg_weights, pooling='max')
    its = []
    torch.manual_seed(0)
    st.stylize(content, styles, style_weights=[0.7, 0.3], optimizer='lbfgs', min_scale=45, end_scale=64, iterations=3,
               initial_iterations=4, callback=lambda it: its.append((it.w, it.h, it.i, it.i_max, it.loss)))
    got, want = np.array(its, dtype=np.float64), g['iterates']
    assert got.shape == want.shape and np.array_equal(got[:, :4], want[:, :4])
    rels = np.abs(got[:, 4] - want[:, 4]) / np.abs(want[:, 4])
    tol = np.maximum(5e-4, 5 * g['trace_spread'])
    print(f'[lbfgs] stylize trace rel {rels} tolerances {tol}')
    assert np.all(rels <= tol)
    d = float((st.get_image_tensor().cpu() - _t(g['result'])).abs().mean())
    print(f'[lbfgs] stylize result mean_abs={d:.3e} (reference self-spread {float(g["result_spread"]):.3e})')
    assert d <= max(1e-4, 5 * float(g['result_spread']))


# ---- 2. the recursion alone, against float64 --------------------------------------------------------------------------
def _objective(shape, dtype, device):
    """|A(x-c)|^2 + 0.05 sum log1p(50 (x_{i+1}-x_i)^2) + 1e-3 |x-c|^2, A Gaussian n/16 x n scaled by n^-1/2 (seeded)."""
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(1)
    A = (torch.randn(n // 16, n, generator=gen, dtype=torch.float64) / n ** 0.5).to(dtype).to(device)
    c = torch.rand(n, generator=gen, dtype=torch.float64).to(dtype).to(device)

    def f(x):
        x = x.detach().reshape(-1).clone().requires_grad_()
        r = A @ (x - c)
        loss = (r * r).sum() + 0.05 * torch.log1p((x[1:] - x[:-1]) ** 2 * 50).sum() + 1e-3 * ((x - c) ** 2).sum()
        loss.backward()
        return loss.detach(), x.grad
    return f, n


def _run_torch(shape, dtype, its, threads):
    before = torch.get_num_threads()
    torch.set_num_threads(threads)
    try:
        f, n = _objective(shape, dtype, 'cpu')
        x = torch.full((n,), 0.5, dtype=dtype, requires_grad=True)
        opt = torch.optim.LBFGS([x], max_iter=1, history_size=10)
        trace = []

        def closure():
            loss, grad = f(x)
            x.grad = grad
            return loss
        for _ in range(its):
            trace.append(float(opt.step(closure)))
    finally:
        torch.set_num_threads(before)
    return np.array(trace), x.detach().double()


@pytest.mark.parametrize('shape', [(3, 64, 64), (3, 57, 68)])
def test_recursion_against_float64(shape):
    """40 iterations (the history of 10 wraps) of st_lbfgs_update on a seeded non-quadratic objective whose gradient torch
    computes; reference torch.optim.LBFGS on the CPU in float64, yardstick torch.optim.LBFGS in fp32 (module docstring)."""
    from style_transfer import _hip
    its = 40
    t64, x64 = _run_torch(shape, torch.float64, its, 8)
    t32a, x32a = _run_torch(shape, torch.float32, its, 1)
    t32b, x32b = _run_torch(shape, torch.float32, its, 8)

    f, n = _objective(shape, torch.float32, DEV)
    x = torch.full(shape, 0.5, device=DEV)
    opt = _hip.LBFGS(x)
    trace, lens = [], []
    for _ in range(its):
        loss, grad = f(x)
        opt.update(x, grad.reshape(shape).contiguous())
        trace.append(float(loss))
        lens.append(opt.info()['history'])
    info = opt.info()
    print(f'[lbfgs] {shape}: history lengths {lens}; final {info}')
    assert info['n_iter'] == its and info['history'] == 10 and lens[:11] == list(range(11)), 'the history must wrap'

    def dev(trace_, x_):
        return np.abs(trace_ - t64) / np.abs(t64), float((x_ - x64).norm() / x64.norm())
    tr_n, x_n = dev(np.array(trace), x.detach().reshape(-1).cpu().double())
    tr_a, x_a = dev(t32a, x32a)
    tr_b, x_b = dev(t32b, x32b)
    floor = n ** 0.5 * 2.0 ** -24
    print(f'[lbfgs] {shape}: loss {t64[0]:.6g} -> {t64[-1]:.6g}; max trace deviation from float64: native {tr_n.max():.3e}, '
          f'torch fp32 1 thread {tr_a.max():.3e}, 8 threads {tr_b.max():.3e}; iterate rel-L2: native {x_n:.3e}, torch fp32 '
          f'{x_a:.3e} / {x_b:.3e}; floor {floor:.2e}')
    assert t64[-1] < 0.5 * t64[0]
    assert np.all(tr_n <= 2 * np.maximum(tr_a, tr_b).max() + floor)
    assert x_n <= 2 * max(x_a, x_b) + floor


# ---- 3. corner cases as exact statements -----------------------------------------------------------------------------
def _torch_lbfgs_on(x0, grads):
    """torch.optim.LBFGS(max_iter=1, history_size=10) on the CPU fed the gradient sequence `grads`; the iterates."""
    x = x0.clone().requires_grad_()
    opt = torch.optim.LBFGS([x], max_iter=1, history_size=10)
    out = []
    for g in grads:
        def closure(g=g):
            x.grad = g.clone()
            return torch.zeros(())
        opt.step(closure)
        out.append(x.detach().clone())
    return out, opt.state[x]


def _native_on(x0, grads, ema=False):
    from style_transfer import _hip
    x = x0.to(DEV).clone()
    opt = _hip.LBFGS(x)
    value = torch.zeros_like(x) if ema else None
    out, infos = [], []
    for g in grads:
        opt.update(x, g.to(DEV), value, 0.99)
        out.append(x.cpu().clone())
        infos.append(opt.info())
    return out, infos, value


@pytest.mark.parametrize('shape', [(3, 16, 16), (3, 19, 17)])      # 16-byte kernels / scalar kernels (odd element count)
def test_zero_gradient_moves_nothing(shape):
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(3))
    got, infos, value = _native_on(x0, [torch.zeros(shape)] * 2, ema=True)
    want, state = _torch_lbfgs_on(x0, [torch.zeros(shape)] * 2)
    assert torch.equal(got[-1], x0) and torch.equal(want[-1], x0)
    assert infos[-1]['n_iter'] == 0 == state.get('n_iter', 0) and infos[-1]['exit'] == 'gradient' and infos[-1]['history'] == 0
    # EMA.update still runs on the unchanged image (reference :486), twice
    e = torch.zeros(shape)
    d = torch.tensor(0.99)
    for _ in range(2):
        e = e * d + (1 - d) * x0
    assert float((value.cpu() - e).abs().max()) <= ULP


@pytest.mark.parametrize('shape', [(3, 16, 16), (3, 19, 17)])
def test_constant_gradient_never_enters_the_history(shape):
    """y = 0 for every pair: ys = 0 fails `ys > 1e-10`, the history stays empty and every step is x -= t g."""
    gen = torch.Generator().manual_seed(4)
    x0 = torch.rand(shape, generator=gen)
    g = torch.rand(shape, generator=gen) - 0.3
    got, infos, _ = _native_on(x0, [g] * 5)
    want, state = _torch_lbfgs_on(x0, [g] * 5)
    assert [i['history'] for i in infos] == [0] * 5 and not any(i['accepted'] for i in infos)
    assert infos[-1]['n_iter'] == 5 == state['n_iter'] and len(state['old_dirs']) == 0
    assert all(i['exit'] == 'moved' for i in infos)
    for k in range(5):
        bound = 4 * ULP * float(want[k].abs().max())          # one axpy per step, each side rounding it once
        assert float((got[k] - want[k]).abs().max()) <= bound, k


def test_small_directional_derivative_keeps_the_image_but_records_s():
    """g.d > -1e-9 on the first step: no move, yet d, t and g_prev are recorded - the second step's pair (y = g1 - g0,
    s = t d) enters the history and its direction equals torch's."""
    shape = (3, 6, 6)                                               # 108 elements of 3e-6: g.g = 9.7e-10 < 1e-9, |g|_inf > 1e-7
    gen = torch.Generator().manual_seed(5)
    x0 = torch.rand(shape, generator=gen)
    g0 = torch.full(shape, 3e-6)
    g1 = -torch.rand(shape, generator=gen) - 0.1
    got, infos, _ = _native_on(x0, [g0, g1])
    want, state = _torch_lbfgs_on(x0, [g0, g1])
    assert torch.equal(want[0], x0), 'the case must not move in torch either'
    assert torch.equal(got[0], x0) and infos[0]['exit'] == 'change' and infos[0]['n_iter'] == 1 and infos[0]['t'] == 1.0
    assert -1e-9 < infos[0]['gtd'] < 0
    assert infos[1]['accepted'] and infos[1]['history'] == 1 == len(state['old_dirs']) and infos[1]['exit'] == 'moved'
    # the pair has |s| = 3e-6 against |y| ~ 1, so H_diag = ys / yy makes the second step a move of ~3e-6: some 50 ulp of the
    # pixels it is added to.  Both sides round that one addition once; their directions differ far below an ulp of x.
    step = float((want[1] - x0).abs().max())
    assert step > 10 * ULP
    assert float((got[1] - want[1]).abs().max()) <= 2 * ULP * float(want[1].abs().max())


@pytest.mark.parametrize('l1', [0.5, 4.0])
def test_first_step_length(l1):
    """t = min(1, 1 / |g|_1) on the first iteration, on both sides of 1."""
    shape = (3, 19, 17)
    gen = torch.Generator().manual_seed(6)
    x0 = torch.rand(shape, generator=gen)
    g = torch.rand(shape, generator=gen) - 0.5
    g = g * (l1 / float(g.abs().sum()))
    got, infos, _ = _native_on(x0, [g])
    want, state = _torch_lbfgs_on(x0, [g])
    t_torch = float(state['t'])
    assert (t_torch == 1.0) == (l1 < 1)
    assert infos[0]['exit'] == 'moved' and abs(infos[0]['t'] - t_torch) <= 4 * ULP * t_torch       # |g|_1 in another order
    assert float((got[0] - want[0]).abs().max()) <= 4 * ULP * float(want[0].abs().max())


# ---- 4. / 5. the full step on a plan ------------------------------------------------------------------------------------
def _plan(hip, weights, size):
    net = hip.Net(weights, 'max', DEV, 'fp16x3')
    plan = hip.Plan(net, size, size)
    content = synth.smooth_image(21, size, size).to(DEV)
    style = synth.smooth_image(22, size, size).to(DEV)
    plan.forward(content, 22)
    plan.set_content_target_from_forward()
    plan.forward(style, 29)
    for i, layer in enumerate([1, 6, 11, 20, 29]):
        plan.set_style_target(i, *plan.moments(layer))
    plan.set_loss_weights(0.015, [256.0, 64.0, 16.0, 4.0, 1.0], 2.0)
    return plan, content


def _native_run(hip, plan, start, its):
    x = start.clone()
    value = (1 - torch.tensor(0.99)).to(DEV) * x
    opt = hip.LBFGS(x)
    losses, iterates = [], []
    for _ in range(its):
        losses.append(opt.step(plan, x, value, 0.99).clone())
        iterates.append(x.clone())
    return x, value, torch.stack(losses), iterates, opt.info()


def test_step_is_deterministic(vgg_weights):
    """12 iterations of st_plan_lbfgs_step at 128^2 twice from the same start: bit-identical image, EMA and losses."""
    from style_transfer import _hip
    plan, content = _plan(_hip, vgg_weights, 128)
    a = _native_run(_hip, plan, content, 12)
    b = _native_run(_hip, plan, content, 12)
    print(f'[lbfgs] 128^2 x 12: total {a[2][:, 7].cpu().numpy()}; {a[4]}')
    assert a[4] == b[4] and a[4]['n_iter'] == 12 and a[4]['history'] == 10
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert float(a[2][-1, 7]) < float(a[2][0, 7])


def test_step_at_512_against_torch_lbfgs(vgg_weights):
    """512^2, 7 iterations from the content image: the native step against torch.optim.LBFGS over the same plan's
    loss_and_grad in the same process - loss traces within 5e-2 relative and both decreasing - and the EMA equal to
    EMA.update applied to the native iterates (<= 1 ulp of fp32 per element)."""
    from style_transfer import _hip
    plan, content = _plan(_hip, vgg_weights, 512)
    x, value, losses, iterates, info = _native_run(_hip, plan, content, 7)
    native = losses[:, 7].cpu().double().numpy()

    y = content.clone().requires_grad_()
    opt = torch.optim.LBFGS([y], max_iter=1, history_size=10)

    def closure():
        with torch.no_grad():
            ls, grad = plan.loss_and_grad(y.detach())
        y.grad = grad
        return ls[7].clone()
    ref = np.array([float(opt.step(closure)) for _ in range(7)])
    rel = np.abs(native - ref) / np.abs(ref)
    print(f'[lbfgs] 512^2: native {native} torch {ref} rel {rel}; {info}')
    assert info['n_iter'] == 7 and info['history'] == 6
    assert np.all(rel <= 5e-2)
    assert native[-1] < native[0] and ref[-1] < ref[0]

    d = torch.tensor(0.99).to(DEV)
    e = (1 - d) * content
    for it in iterates:
        e = e * d
        e = e + (1 - d) * it
    err = (value - e).abs()
    assert bool((err <= ULP * e.abs().clamp_min(2.0 ** -126)).all()), float(err.max())
