"""optimizer='lbfgs' on row strips as the native vector-free step (st_qn_strip_* / st_plan_qn_strip_step in
include/st_amd.h, csrc/st_lbfgs.hip) on a real MI355X: per iteration every rank writes a record of 70 sums and one
maximum, ONE all-gather hands every rank every record, and every rank adds them in rank order in double.  One GPU executes
of that: several ranks' states in one process with the gather as device copies (sharding.lbfgs_lockstep), the in-library
RCCL all-gather on one rank, and two OS processes on cuda:0 over gloo.

Tolerances and where they come from:
  * one strip: the sum of one record is that record, so the step is st_lbfgs_update bit for bit;
  * the recursion against float64: the bar of tests/test_lbfgs_gpu.py::test_recursion_against_float64, measured inside the
    test - no further from torch.optim.LBFGS in float64 than 2 x torch's own fp32 runs (1 and 8 threads), plus the floor
    sqrt(n) 2^-24 of one fp32 evaluation of a sum of n terms;
  * decisions: exact statements (bits, counters, flags); iterates and t to 4 ulp of fp32 where one axpy / one sum differs
    in its rounding only;
  * stylize() on two ranks: the 5e-2 relative loss trace / 5e-3 mean absolute image of
    tests/test_stylize_sharded_gpu.py::test_stylize_lbfgs_in_separate_processes_matches_single_gpu.
"""
import functools
import os
import subprocess
import sys
import traceback

import numpy as np
import pytest
import torch

from test_lbfgs_gpu import _objective, _run_torch, _torch_lbfgs_on

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
ULP = 2.0 ** -23
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _cut(flat, sizes):
    """Segments of a flat vector as tensors of their own (own allocations: every segment 16-byte aligned)."""
    assert sum(sizes) == flat.numel()
    return [seg.clone() for seg in flat.reshape(-1).split(list(sizes))]


def _strips(x0, sizes):
    from style_transfer import _hip
    xs = _cut(x0.to(DEV), sizes)
    opts = [_hip.LBFGS(x, r, len(sizes)) for r, x in enumerate(xs)]
    emas = [torch.zeros_like(x) for x in xs]
    return xs, opts, emas


def _strips_on(x0, grads, sizes):
    """The lockstep strips fed the gradient sequence `grads` (whole flat vectors): per step the whole iterate (CPU) and
    every rank's info(); the EMA at the end."""
    from style_transfer import sharding
    xs, opts, emas = _strips(x0, sizes)
    out, infos = [], []
    for g in grads:
        sharding.lbfgs_lockstep(opts, xs, _cut(g.to(DEV), sizes), emas, 0.99)
        out.append(torch.cat(xs).cpu())
        infos.append([o.info() for o in opts])
    return out, infos, torch.cat(emas).cpu()


# ---- 1. one strip is the unsharded step ----------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', [(3, 16, 16), (3, 19, 17)])      # 16-byte kernels / scalar kernels (odd element count)
def test_one_strip_is_the_unsharded_step(shape):
    """world = 1 through the lockstep helper, 14 iterations (the history wraps at the 11th): image, EMA and info() are
    bit-identical to _hip.LBFGS.update fed the same gradients."""
    from style_transfer import _hip, sharding
    f, n = _objective(shape, torch.float32, DEV)
    x = torch.full(shape, 0.5, device=DEV)
    y = x.clone()
    ex, ey = torch.zeros_like(x), torch.zeros_like(y)
    ref, opt = _hip.LBFGS(x), _hip.LBFGS(y, 0, 1)
    lens = []
    for it in range(14):
        _, grad = f(x)
        grad = grad.reshape(shape).contiguous()
        ref.update(x, grad, ex, 0.99)
        sharding.lbfgs_lockstep([opt], [y], [grad], [ey], 0.99)
        a, b = ref.info(), opt.info()
        lens.append(b['history'])
        assert a == b, (it, a, b)
        assert torch.equal(x, y) and torch.equal(ex, ey), it
    print(f'[lbfgs-strips] {shape}: one strip, history lengths {lens}, final {opt.info()}')
    assert lens[:11] == list(range(11)) and lens[-1] == 10 and opt.info()['n_iter'] == 14


# ---- 2. the recursion on strips against float64 ------------------------------------------------------------------------------
SHAPE = (3, 57, 68)                                      # 11 628 elements
CUTS = {3: (4099, 3529, 4000), 2: (5814, 5814)}         # odd counts: scalar kernels; multiples of 4: 16-byte kernels
ITS = 40


@functools.lru_cache(maxsize=None)
def _torch_references():
    """torch.optim.LBFGS on the CPU: float64 (the reference) and fp32 at 1 and 8 threads (the yardstick); computed once."""
    return (_run_torch(SHAPE, torch.float64, ITS, 8), _run_torch(SHAPE, torch.float32, ITS, 1),
            _run_torch(SHAPE, torch.float32, ITS, 8))


def _strip_recursion(sizes):
    from style_transfer import sharding
    f, n = _objective(SHAPE, torch.float32, DEV)
    xs, opts, emas = _strips(torch.full((n,), 0.5), sizes)
    trace, lens = [], []
    for it in range(ITS):
        loss, grad = f(torch.cat(xs))                    # the gradient of the whole vector, computed by torch and cut
        sharding.lbfgs_lockstep(opts, xs, _cut(grad, sizes), emas, 0.99)
        trace.append(float(loss))
        infos = [o.info() for o in opts]
        assert all(i == infos[0] for i in infos), (it, infos)      # t, gtd equal as doubles, every flag and counter
        lens.append(infos[0]['history'])
    return np.array(trace), torch.cat(xs), torch.cat(emas), lens, infos[0]


@functools.lru_cache(maxsize=None)
def _strip_recursion_once(world):
    return _strip_recursion(CUTS[world])


@pytest.mark.parametrize('world', [3, 2])
def test_recursion_on_strips_against_float64(world):
    (t64, x64), (t32a, x32a), (t32b, x32b) = _torch_references()
    trace, x, _, lens, info = _strip_recursion_once(world)
    n = x.numel()
    print(f'[lbfgs-strips] {CUTS[world]}: history lengths {lens}; final {info}')
    assert info['n_iter'] == ITS and lens[:11] == list(range(11)) and all(v == 10 for v in lens[10:]), 'the history must wrap'

    def dev(trace_, x_):
        return np.abs(trace_ - t64) / np.abs(t64), float((x_ - x64).norm() / x64.norm())
    tr_n, x_n = dev(trace, x.cpu().double())
    tr_a, x_a = dev(t32a, x32a)
    tr_b, x_b = dev(t32b, x32b)
    floor = n ** 0.5 * 2.0 ** -24
    print(f'[lbfgs-strips] {CUTS[world]}: loss {t64[0]:.6g} -> {t64[-1]:.6g}; max trace deviation from float64: strips '
          f'{tr_n.max():.3e}, torch fp32 1 thread {tr_a.max():.3e}, 8 threads {tr_b.max():.3e}; iterate rel-L2: strips {x_n:.3e}, '
          f'torch fp32 {x_a:.3e} / {x_b:.3e}; floor {floor:.2e}')
    assert t64[-1] < 0.5 * t64[0]
    assert np.all(tr_n <= 2 * np.maximum(tr_a, tr_b).max() + floor)
    assert x_n <= 2 * max(x_a, x_b) + floor


# ---- 4. run to run -------------------------------------------------------------------------------------------------------
def test_strips_are_deterministic():
    """The three-strip case twice from the same start: iterates, EMAs and info() bit-identical (every sum is formed in a
    fixed order: within a workgroup, over the workgroups, over the ranks)."""
    a = _strip_recursion_once(3)
    b = _strip_recursion(CUTS[3])
    assert np.array_equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and a[3] == b[3] and a[4] == b[4]


# ---- 3. decisions are global -----------------------------------------------------------------------------------------------
N, HALVES = 969, (485, 484)                              # 3 x 19 x 17 cut into a scalar-kernel and a 16-byte-kernel strip


def test_zero_gradient_everywhere_moves_nothing():
    x0 = torch.rand(N, generator=torch.Generator().manual_seed(3))
    got, infos, value = _strips_on(x0, [torch.zeros(N)] * 2, HALVES)
    want, state = _torch_lbfgs_on(x0, [torch.zeros(N)] * 2)
    assert torch.equal(got[-1], x0) and torch.equal(want[-1], x0)
    for info in infos[-1]:
        assert info['n_iter'] == 0 == state.get('n_iter', 0) and info['exit'] == 'gradient' and info['history'] == 0
    e = torch.zeros(N)                                   # EMA.update still runs on the unchanged image, twice
    d = torch.tensor(0.99)
    for _ in range(2):
        e = e * d + (1 - d) * x0
    assert float((value - e).abs().max()) <= ULP


def test_a_strip_with_zero_gradient_follows_the_global_decision():
    """|g|_inf = 0 on rank 0 alone would be the tolerance_grad return; the maximum over the ranks is not."""
    gen = torch.Generator().manual_seed(4)
    x0 = torch.rand(N, generator=gen)
    g = torch.cat([torch.zeros(HALVES[0]), torch.rand(HALVES[1], generator=gen) - 0.3])
    got, infos, _ = _strips_on(x0, [g], HALVES)
    want, state = _torch_lbfgs_on(x0, [g])
    assert all(i['exit'] == 'moved' and i['n_iter'] == 1 for i in infos[0]) and state['n_iter'] == 1
    assert infos[0][0] == infos[0][1]
    assert torch.equal(got[0][:HALVES[0]], x0[:HALVES[0]]), 'd = 0 on the strip without gradient'
    assert not torch.equal(want[0][HALVES[0]:], x0[HALVES[0]:])
    bound = 4 * ULP * float(want[0].abs().max())          # one axpy, each side rounding it once; t from |g|_1 in another order
    assert float((got[0] - want[0]).abs().max()) <= bound


def test_directional_derivative_is_summed_over_the_strips():
    """216 elements of 3e-6 cut 108 / 108: each half alone has g.g = 9.7e-10 < 1e-9 (the `change` exit of the unsharded
    108-element test), together 1.94e-9: both ranks move, as torch does on the whole vector.  The 108-element case itself cut
    60 / 48 takes the `change` exit on both ranks and leaves the image alone."""
    gen = torch.Generator().manual_seed(5)
    x0 = torch.rand(216, generator=gen)
    g = torch.full((216,), 3e-6)
    got, infos, _ = _strips_on(x0, [g], (108, 108))
    want, state = _torch_lbfgs_on(x0, [g])
    assert not torch.equal(want[0], x0), 'the case must move in torch'
    assert all(i['exit'] == 'moved' and i['n_iter'] == 1 and i['t'] == 1.0 for i in infos[0]) and infos[0][0] == infos[0][1]
    assert -2e-9 < infos[0][0]['gtd'] < -1.9e-9
    assert float((got[0] - want[0]).abs().max()) <= 4 * ULP * float(want[0].abs().max())

    got, infos, _ = _strips_on(x0[:108], [g[:108]], (60, 48))
    want, state = _torch_lbfgs_on(x0[:108], [g[:108]])
    assert torch.equal(want[0], x0[:108]) and torch.equal(got[0], x0[:108])
    assert all(i['exit'] == 'change' and i['n_iter'] == 1 for i in infos[0]) and infos[0][0] == infos[0][1]
    assert -1e-9 < infos[0][0]['gtd'] < 0


def test_first_step_length_uses_the_global_l1_norm():
    """Local |g|_1 = 0.6 on both strips: min(1, 1 / 0.6) = 1 on either alone, t = 1 / 1.2 on the whole vector."""
    gen = torch.Generator().manual_seed(6)
    x0 = torch.rand(N, generator=gen)
    g = torch.rand(N, generator=gen) - 0.5
    g = torch.cat([s * (0.6 / float(s.abs().sum())) for s in g.split(list(HALVES))])
    got, infos, _ = _strips_on(x0, [g], HALVES)
    want, state = _torch_lbfgs_on(x0, [g])
    t_torch = float(state['t'])
    assert abs(t_torch - 1 / 1.2) < 1e-5 and t_torch != 1.0
    for info in infos[0]:
        assert info['exit'] == 'moved' and info['t'] != 1.0 and abs(info['t'] - t_torch) <= 4 * ULP * t_torch
    assert infos[0][0] == infos[0][1]
    assert float((got[0] - want[0]).abs().max()) <= 4 * ULP * float(want[0].abs().max())


# ---- 5. the in-library RCCL all-gather on one rank ----------------------------------------------------------------------------
CHILD = r'''
import ctypes, os, sys
sys.path.insert(0, os.path.join(%(root)r, 'style-transfer-pytorch_amd'))
sys.path.insert(0, os.path.join(%(root)r, 'tests'))
import torch
import synth
from style_transfer import _hip, sharding, vgg

H, W, ITS = 64, 48, 6
dev = torch.device('cuda', 0)
torch.cuda.set_device(dev)
net = _hip.Net(vgg.synthetic_vgg19_weights(0), 'max', dev, 'fp16x3')
content, style = synth.smooth_image(21, H, W).to(dev), synth.smooth_image(22, H, W).to(dev)
native = sharding.NativeFabric(0, 1, dev, cold=sharding.DistFabric(0, 1))      # (its constructor runs st_fabric_selftest)
assert native.lib.st_fabric_selftest(native.handle, _hip._stream(), 30000) == 0, native.lib.st_last_error()
print('[lbfgs-strips] st_fabric_selftest passed with the all-gather in it', flush=True)
plan = sharding.StripPlan(net, H, W, 0, H).set_rank(0, 1)                       # ONE strip: the whole image
sharding.set_targets(plan, content, [style], [1.0], lambda p: sharding.run_phases(p, native), lambda t: None)
plan.set_loss_weights(0.015, [w / 341 for w in (256, 64, 16, 4, 1)], 2.0)

def run(one_call):
    x = content.clone()
    grad = torch.empty_like(x)
    ema = (1 - torch.tensor(0.99)).to(dev) * x
    opt = _hip.LBFGS(x, 0, 1)
    losses, infos = [], []
    for _ in range(ITS):
        if one_call:                                     # st_plan_qn_strip_step: closure, dots, ncclAllGather, apply in one call
            opt.step_strip(plan, native, x, grad, ema, 0.99)
        else:                                            # the unsharded update behind the same closure
            plan.closure_begin(x, grad)
            sharding.run_phases(plan, native)
            opt.update(x, grad, ema, 0.99)
        losses.append(plan.losses.clone())
        infos.append(opt.info())
    return x, ema, torch.stack(losses), infos

a, b = run(True), run(False)
print('[lbfgs-strips] one-call strip step over RCCL: total', a[2][:, 7].cpu().numpy(), a[3][-1], flush=True)
assert a[3] == b[3], (a[3], b[3])
assert a[3][-1]['n_iter'] == ITS and a[3][-1]['exit'] == 'moved'
assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
assert not torch.equal(a[0], content) and float(a[2][-1, 7]) < float(a[2][0, 7])
torch.cuda.synchronize()
native.close()
print('[lbfgs-strips] RCCL OK', flush=True)
'''


def test_one_call_step_over_the_in_library_transport():
    """st_plan_qn_strip_step on a NativeFabric of one rank (a StripPlan that covers the whole 64 x 48 image, 6 iterations,
    a real ncclAllGather per iteration) against closure_begin + run_phases + _hip.LBFGS.update on a second image from the
    same start: image, EMA, losses and info() bit-identical; st_fabric_selftest passes with the all-gather in it.  In a child
    process with a hard timeout, as tests/test_rccl_self_halo_gpu.py."""
    env = dict(os.environ, ST_FABRIC_FORCE_COLLECTIVES='1')
    r = subprocess.run([sys.executable, '-c', CHILD % {'root': ROOT}], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert '[lbfgs-strips] RCCL OK' in r.stdout


# ---- 6. stylize() on two ranks --------------------------------------------------------------------------------------------
LBFGS_KW = dict(optimizer='lbfgs', iterations=3, initial_iterations=4)


def _worker(rank, world, port, out):
    try:
        sys.path.insert(0, os.path.join(HERE, '..', 'style-transfer-pytorch_amd'))
        sys.path.insert(0, HERE)
        import torch.distributed as dist
        import style_transfer as st_pkg
        from style_transfer import sharding, vgg
        from test_stylize_sharded_gpu import KW, _pil

        def refuse(*a, **k):
            raise AssertionError('the iteration left the native strip step')
        torch.optim.LBFGS = refuse
        sharding.StripLBFGS.__init__ = refuse
        dev = torch.device('cuda', 0)
        torch.cuda.set_device(dev)
        dist.init_process_group('gloo', init_method=f'tcp://127.0.0.1:{port}', rank=rank, world_size=world)
        weights = vgg.synthetic_vgg19_weights(0)
        kw = dict(KW, **LBFGS_KW)
        content, styles = _pil(1, 96, 80), [_pil(2, 120, 90), _pil(3, 28, 40)]
        trace = []
        st = st_pkg.StyleTransfer(devices=['cuda:0'], weights=weights)
        st.stylize(content, styles, callback=lambda it: trace.append((it.w, it.h, it.i, it.loss)), **kw)
        result = st.get_image_tensor().cpu()
        torch.cuda.synchronize()
        gathered = [torch.empty_like(result) for _ in range(world)] if rank == 0 else None
        dist.gather(result, gathered, dst=0)
        dist.barrier()
        dist.destroy_process_group()
        if rank == 0:
            same = all(torch.equal(g, gathered[0]) for g in gathered)
            trace1 = []
            st1 = st_pkg.StyleTransfer(devices=['cuda:0'], weights=weights)     # no process group: single-GPU path
            st1.stylize(content, styles, callback=lambda it: trace1.append((it.w, it.h, it.i, it.loss)), **kw)
            diff = (result - st1.get_image_tensor().cpu()).abs()
            out.put(('ok', same, float(diff.mean()), float(diff.max()), trace, trace1, tuple(result.shape)))
    except Exception:                            # noqa: BLE001 - reported to the parent
        out.put(('error', rank, traceback.format_exc()))
        raise


def test_stylize_lbfgs_on_two_ranks_is_the_native_strip_step():
    """Two OS processes on cuda:0 over gloo, the images and the call of
    test_stylize_sharded_gpu.py::test_stylize_lbfgs_in_separate_processes_matches_single_gpu, with torch.optim.LBFGS and
    sharding.StripLBFGS made to raise: the run completes on the native strip step (descriptor form: dots, all-gather
    through DistFabric.apply, apply), the gathered result is bit-identical on both ranks and follows the single-process run
    (the unsharded native step) within that test's bars."""
    import torch.multiprocessing as mp
    from test_stylize_sharded_gpu import _free_port
    ctx = mp.get_context('spawn')
    out = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, out)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=420)
    alive = [p for p in procs if p.is_alive()]
    for p in alive:
        p.kill()                                 # exact handles of the processes started above
    assert not alive, 'a rank hung'
    results = []
    while not out.empty():
        results.append(out.get())
    errors = [r for r in results if r[0] == 'error']
    assert not errors, errors[0][2]
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    (_, same, mean_abs, max_abs, trace, trace1, shape), = [r for r in results if r[0] == 'ok']
    assert shape == (3, 96, 80) and [t[:3] for t in trace] == [t[:3] for t in trace1], 'same scales and iteration counts'
    rels = [abs(a[3] - b[3]) / abs(b[3]) for a, b in zip(trace, trace1)]
    print(f'[lbfgs-strips] stylize R=2: identical across ranks {same}, image mean_abs {mean_abs:.2e} max_abs {max_abs:.2e}, '
          f'loss-trace rel diffs {["%.1e" % r for r in rels]}')
    assert same, 'every rank must hold the same gathered result'
    assert max(rels) <= 5e-2 and mean_abs <= 5e-3
