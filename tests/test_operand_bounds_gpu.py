"""Every fp16x3 operand bound against the tensor it describes, on a real MI355X.

The 3 x 3 trunk convolutions, their data gradients, the Gram kernels and the heads' 1 x 1 step stage their operand as fp16
planes scaled by a power of two taken from a device word, which the PRODUCER of the operand raised to max |operand| while it
wrote it (csrc/st_common.h: amax_commit, scale_exp).  A word that is too small by up to two binades, or too large by any
number of them, changes no result that another test looks at: fp16 has two spare bits above the scaled bound, and a loose
bound only raises an underflow floor far below every bar of the suite.  Here the 64 words of a plan are read back
(``Plan.debug_read(2, 64)``, include/st_amd.h) after every kind of pass and held against the tensors they are documented to
bound.

The invariant.  A consumer that reads the word b assumes max |T| < B = 2^(floor(log2 b) + 1) (B = 0 for b = 0).  With m =
max |T| over the tensor(s) the word bounds, in the form the consumer stages them (a gradient: already multiplied by its
ReLU's mask):
    never under   B > m (1 - tau); a pooled map on its input's word under average / L2 pooling: 2 B > m (1 - tau), the
                  spare bit scale_exp documents
    never loose   B <= 2 m (1 + tau), wherever the kernel that writes the final tensor commits the word (LOOSE_EXEMPT names
                  the words where an earlier launch of the pass commits as well, with the launch)
    unused        a word no launch of the pass uses reads 0
m comes from the device's own map where the pass leaves one (``Plan.feature``, ``Plan.debug_read(16 + i, n)``): tau = 0, the
exponents must agree exactly.  Otherwise from the float64 oracle on the plan's own branches, with tau = 1/16: far above the
fp32-class error of a single element (3e-6 on maps, 1e-3 on gradients are the suite's bars), far below the factor >= 2 that
a forgotten maximum costs in the inputs below.

The inputs.  On random or smooth inputs a producer that forgets part of its tile when it folds the maximum passes: the
maximum is practically never in the forgotten part.  So the network here has centre-dominant weights (centre tap 1 from
input channel o % cin to output channel o, plus a small He-scaled perturbation and small biases), under which one pixel of
8 x the image's range is the maximum of every map at that pixel >> level, and a cotangent spike at a tap is the maximum of
every gradient map below it; the spike is moved over the borders, the diagonals and the last row / column of every level of
a 75 x 107 image (ragged at all five levels: 75 x 107, 37 x 53, 18 x 26, 9 x 13, 4 x 6).  That the spike dominates by a factor
>= 2 wherever the oracle is the reference is asserted on the CPU first.  The 4 x 4-aligned kernels (conv1_1's four-pixel and
Gram kernels, the fat tile, the fused max pool and the argmax-coded forward) never run at a width of 107: they get a
76 x 128 image, and conv1_2 / conv2_2's two-launch cover a 362 x 362 one.

The heads' own words (48 ... 63, and the regions' block) bound the C x C matrices Ssym, which no entry point reads back: they
are checked for use (a listed head's word is set by a closure, every other one reads 0), not against the matrix;
tests/test_native_losses_gpu.py moves the stand-alone head's bound by ten binades.  Strip plans carry their halo bounds in the
message (test_halo_bounds_travel_with_the_rows).
"""
import functools
import math

import pytest
import torch

import st_oracle as O
import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = (75, 107)             # ragged at all five levels
ALIGNED = (76, 128)          # widths that are multiples of 4 down to 8, heights 76 38 19 9 4: the 16-byte store paths
COVER = (362, 362)           # conv1_2 / conv2_2 in two launches (test_conv_pc_two_shape_cover's shapes)
TAU = 1.0 / 16               # against the float64 oracle (module docstring); 0 against the device's own maps
AMP = 8.0                    # the spike, in units of the image's range
DOMINANCE = 2.0              # CPU precondition: the spike's pixel over every other pixel of a bounded tensor
PERTURBATION, BIAS = 0.05, 0.02      # tuned on the CPU until both preconditions held with room (ratios 3.7 ... 13 at 75 x 107)

# the 17 taps in network order (kProgram), their y / g words (st_api.hip: plan_create_common) and pooling level
TAPS, RELUS, POOLS, Y_WORD, G_WORD, LEVEL = [], [], [], {}, {}, {}
_conv, _level = -1, 0
for _idx, _op, _n in O.layer_program():
    if _op == 'conv':
        _conv = _n
    elif _op == 'relu':
        TAPS.append(_idx), RELUS.append(_idx)
        Y_WORD[_idx], G_WORD[_idx], LEVEL[_idx] = _conv, 16 + _conv, _level
    else:
        _level += 1
        TAPS.append(_idx), POOLS.append(_idx)
        Y_WORD[_idx], LEVEL[_idx] = _conv, _level                   # a pooled map reuses its input's y word
        G_WORD[_idx] = G_WORD[_idx - 1] = 32 + len(POOLS) - 1       # a convolution that feeds a pool reuses the pool's g word
G_WORDS = sorted(set(G_WORD.values()))
HEAD_WORDS = range(48, 64)
NEVER_USED = [w for w in range(64) if w not in set(Y_WORD.values()) and w not in G_WORDS and w not in HEAD_WORDS]

# Words exempt from the never-loose half, by configuration, with the launch that is the reason.  profiles/operand_bounds.md
# records the same list.
LOOSE_EXEMPT = {
    # the default closure's style heads write their tap's gradient buffer themselves and commit max |dF| of their own term
    # (style_head_gradient: head_step with grad_amax); the data gradient of the convolution above then ADDS onto the buffer
    # and applies the ReLU mask (dgrad_conv: accumulate + out_mask), so the final tensor may be smaller than what the head
    # committed.  relu5_1's head (word 28) writes the final, masked gradient: not exempt.
    'default closure': {16: "relu1_1's head_step commits before conv1_2's data gradient accumulates and masks",
                        18: "relu2_1's head_step commits before conv2_2's data gradient accumulates and masks",
                        20: "relu3_1's head_step commits before conv3_2's data gradient accumulates and masks",
                        24: "relu4_1's head_step commits before conv4_2's data gradient accumulates and masks"},
    # st_plan_forward, st_plan_backward and the general closure (other taps, Gram heads, a style mask, regions): every word is
    # committed by the launch that writes the final tensor - the general closure's heads write seed buffers without a bound,
    # mask_columns_kernel scales those, and run_tap_backward's seeding launch commits afterwards
    'forward': {}, 'backward': {}, 'general closure': {},
}


def _hip():
    from style_transfer import _hip as hip
    return hip


@functools.lru_cache(maxsize=None)
def centre_weights():
    """13 (weight, bias) pairs: identity on the centre tap from input channel o % cin, a seeded He-scaled perturbation of
    PERTURBATION on every tap, biases in +-BIAS."""
    g = torch.Generator().manual_seed(5)
    out, cin = [], 3
    for cout in (c for c in O._CFG if c != 'M'):
        w = torch.randn((cout, cin, 3, 3), generator=g) * (PERTURBATION * (2.0 / (9 * cin)) ** 0.5)
        o = torch.arange(cout)
        w[o, o % cin, 1, 1] += 1.0
        out.append((w.contiguous(), (torch.rand(cout, generator=g) - 0.5) * (2 * BIAS)))
        cin = cout
    return out


@functools.lru_cache(maxsize=None)
def centre_weights64():
    return [(w.double(), b.double()) for w, b in centre_weights()]


@functools.lru_cache(maxsize=None)
def base_image(size, seed=91):
    return synth.smooth_image(seed, *size)


def spiked(image, y, x, amp=AMP):
    out = image.clone()
    out[0, :, y, x] = amp
    return out


def make_plan(size, pooling='max'):
    hip = _hip()
    net = hip.Net(centre_weights(), pooling, DEV, 'fp16x3')
    wide = net.wide_layers()
    assert not any(wide[0]) and not any(wide[1]), f'the range guard moved layers to bf16x6 {wide}: fp16x3 is not under test'
    return net, hip.Plan(net, *size)


# ---- the invariant ---------------------------------------------------------------------------------------------------------
def limit(b):
    """B = 2^(floor(log2 b) + 1): the exclusive limit a consumer of the bound b assumes; 0 for b = 0."""
    if b == 0:
        return 0.0
    return 2.0 ** math.frexp(b)[1]          # b = f 2^e with f in [0.5, 1)


def bound_failures(name, b, m, tau=0.0, loose=True, spare=1):
    """The invariant for one word with read-out ``b`` and one m = max |T|; a list of messages, empty when it holds."""
    if not (math.isfinite(b) and b >= 0 and math.isfinite(m)):
        return [f'{name}: bound {b!r}, max |T| {m!r}']
    big, out = limit(b), []
    if m > 0 and not spare * big > m * (1 - tau):
        out.append(f'{name}: UNDER, B = {big:g} (x {spare} spare) against max |T| = {m:g}')
    if loose and not big <= 2 * m * (1 + tau):
        out.append(f'{name}: LOOSE, B = {big:g} against max |T| = {m:g}')
    return out


class Slack:
    """The largest looseness seen, in binades: log2 of B over the smallest power of two above max |T|."""

    def __init__(self, name):
        self.name, self.worst, self.where, self.exempt = name, -math.inf, '', {}

    def see(self, word, b, m, exempt=False):
        if b > 0 and m > 0:
            s = math.log2(limit(b)) - math.log2(limit(m))
            if exempt:
                self.exempt[word] = max(s, self.exempt.get(word, -math.inf))
            elif s > self.worst:
                self.worst, self.where = s, f'word {word}'

    def report(self):
        exempt = ''.join(f', exempt word {w} {s:+.0f}' for w, s in sorted(self.exempt.items()))
        print(f'[bounds] {self.name}: largest looseness {self.worst:+.0f} binades ({self.where}){exempt}')


def zero_failures(words, which, where):
    return [f'{where} word {w}: unused, reads {words[w]!r}' for w in which if words[w] != 0]


def device_amax(tensors):
    if not tensors:
        return []
    return torch.stack([t.abs().max() for t in tensors]).cpu().tolist()


def forward_failures(plan, pooling, last_layer, where, slack, y_reference=None, skip_device=()):
    """After a pass that ran the forward up to ``last_layer``: words 0 .. 12 against the device's maps (both halves, exact
    exponents; a pooled map: never under, on its input's word), or against ``y_reference`` ({layer: max |y|} in float64,
    tau = 1/16) as well; the y words beyond ``last_layer`` read 0.  ``skip_device``: ReLU outputs the pass did not write."""
    words = plan.debug_read(2, 64).tolist()
    layers = [t for t in TAPS if t <= last_layer and t not in skip_device]
    amax = dict(zip(layers, device_amax([plan.feature(t) for t in layers])))
    out = []
    for layer in RELUS:
        word = Y_WORD[layer]
        if layer > last_layer:
            out += zero_failures(words, [word], where)
            continue
        if layer in amax:
            out += bound_failures(f'{where} y word {word} (features[{layer}], device map)', words[word], amax[layer])
            slack.see(word, words[word], amax[layer])
        if y_reference is not None:
            out += bound_failures(f'{where} y word {word} (features[{layer}], float64)', words[word], y_reference[layer], TAU)
    for layer in POOLS:
        if layer <= last_layer:
            out += bound_failures(f'{where} y word {Y_WORD[layer]} (pooled features[{layer}])', words[Y_WORD[layer]], amax[layer],
                                  loose=False, spare=1 if pooling == 'max' else 2)
    return words, out


def assert_none(failures, what):
    assert not failures, f'{what}: {len(failures)} failures\n  ' + '\n  '.join(failures[:40])


# ---- spike positions -------------------------------------------------------------------------------------------------------
def level_edges(n):
    """((n >> l) - 1) << l for the five levels: the first pixel of the last row / column of level l."""
    return sorted({((n >> lv) - 1) << lv for lv in range(5)})


def border(h, w):
    return sorted({(y, x) for y in (0, h - 1) for x in range(w)} | {(y, x) for y in range(h) for x in (0, w - 1)})


def sweep(h, w):
    """Every pixel of the first and last row and column, both diagonals, and the rows and columns that are the last of a level."""
    pos = set(border(h, w))
    for y in range(h):
        x = round(y * (w - 1) / (h - 1))
        pos |= {(y, x), (y, w - 1 - x)}
    for y in level_edges(h):
        pos |= {(y, x) for x in range(w)}
    for x in level_edges(w):
        pos |= {(y, x) for y in range(h)}
    return sorted(pos)


def coarse(h, w):
    """The corners, the crossings of the levels' last rows and columns, and the middle of each edge."""
    ys, xs = sorted({0, h // 2, h - 1, *level_edges(h)}), sorted({0, w // 2, w - 1, *level_edges(w)})
    return [(y, x) for y in ys for x in xs]


def forward_sweep(size, pooling, positions, name, last_layer=29, amp=AMP, prepare=None):
    net, plan = make_plan(size, pooling)
    base = base_image(size).to(DEV)
    if prepare:
        prepare(plan, base)
    slack, failures = Slack(name), []
    for y, x in positions:
        plan.forward(spiked(base, y, x, amp), last_layer)
        words, bad = forward_failures(plan, pooling, last_layer, f'{name} spike ({y}, {x})', slack)
        failures += bad + zero_failures(words, [w for w in range(13, 64)], f'{name} spike ({y}, {x})')
    slack.report()
    print(f'[bounds] {name}: {len(positions)} spike positions, {len(failures)} failures')
    assert_none(failures, name)


# ---- forward ---------------------------------------------------------------------------------------------------------------
def test_forward_border_and_diagonal_sweep():
    """Plan.forward(img, 29), max pooling: the spike on every pixel of the border, of both diagonals and of each level's last
    row and column (a spike in the odd last row of level 0 disappears at pool 1: the deeper words must then be the rest's)."""
    forward_sweep(SIZE, 'max', sweep(*SIZE), 'forward 75x107 max')


@pytest.mark.parametrize('last_layer', [1, 3, 4, 8, 18, 22, 27])
def test_forward_stops_at_last_layer(last_layer):
    """... and with the forward cut short: the words of the convolutions beyond it read 0."""
    forward_sweep(SIZE, 'max', coarse(*SIZE), f'forward 75x107 max last_layer {last_layer}', last_layer)


@pytest.mark.parametrize('pooling', ['average', 'l2'])
def test_forward_average_and_l2_pooling_share_the_word_with_the_spare_bit(pooling):
    """Average (x 2) and L2 (x 0.78) pooling: a pooled map may exceed its input's bound by less than a binade.  (The spike is
    8 x 16: an average pool halves an isolated pixel at every level.)"""
    forward_sweep(SIZE, pooling, coarse(*SIZE), f'forward 75x107 {pooling}', amp=AMP * 16)


# which kernel produced the map: the switches that change the producing kernel (st_set_option; a default build honours them)
def _pc_forced():
    cases = [dict(ST_CONV_PC=0)]                                                            # the single-role split kernel
    cases.append(dict(ST_CONV_PC=2, ST_CONV_PC_SHAPE=1, ST_CONV_PC_TW=32, ST_CONV_PC_KSPLIT=1))      # the XL tile
    for shape in (2, 3):                                                                    # 256- and 128-pixel tiles
        for tw in (32, 16, 8):
            for ks in (1, 2):       # K split 2: the split-K reduce is the committing kernel (conv1_2 has 4 K chunks: no more)
                cases.append(dict(ST_CONV_PC=2, ST_CONV_PC_SHAPE=shape, ST_CONV_PC_TW=tw, ST_CONV_PC_KSPLIT=ks))
    cases.append(dict(ST_CONV_PC=2, ST_CONV_PC_MODEL=0))                                    # the round-1 tile rule
    cases.append(dict(ST_CONV_POOL_FUSE=0))
    return cases


def _opts_id(opts):
    return '-'.join(f'{k[3:]}={v}' for k, v in opts.items())


@pytest.mark.parametrize('opts', _pc_forced(), ids=_opts_id)
def test_forward_border_sweep_by_producing_kernel(opts):
    """The border sweep with the 3 x 3 producer forced: the single-role kernel, every producer / consumer tile in its three
    widths, without and with a K split (as test_conv_pc_forced_tiles forces them)."""
    with _hip().options(**opts):
        forward_sweep(SIZE, 'max', border(*SIZE), f'forward 75x107 {_opts_id(opts)}')


ALIGNED_KERNELS = [dict(), dict(ST_CONV_FAT=2), dict(ST_CONV_FAT=2, ST_CONV_FAT_CB=2), dict(ST_CONV1_WIDE=0),
                   dict(ST_CONV_POOL_FUSE=0), dict(ST_CONV_PC=0)]


@pytest.mark.parametrize('opts', ALIGNED_KERNELS, ids=lambda o: _opts_id(o) or 'default')
def test_forward_border_sweep_aligned_kernels(opts):
    """76 x 128, where the 16-byte paths apply: conv1_1's four-pixel kernel (default) and its one-pixel kernel, the fused max
    pool of the producer / consumer epilogue, and the fat tile forced onto every layer it takes (as
    test_fat_conv_kernel_in_the_closure_is_bit_identical forces it)."""
    with _hip().options(**opts):
        forward_sweep(ALIGNED, 'max', border(*ALIGNED), f'forward 76x128 {_opts_id(opts) or "default"}')


def test_forward_border_sweep_conv1_1_gram_kernel():
    """conv1_1's third forward kernel, which also leaves relu1_1's partial moments (ST_CONV1_GRAM=1, through st_plan_forward
    as tests/test_kernels_gpu.py runs it): it commits relu1_1's word itself."""
    def prepare(plan, base):
        plan.forward(base, 1)
        plan.moments(1)                 # relu1_1's head gets its moment buffers: the fused kernel needs them
    with _hip().options(ST_CONV1_GRAM_IN_FORWARD=1, ST_CONV1_GRAM=1):
        forward_sweep(ALIGNED, 'max', border(*ALIGNED), 'forward 76x128 conv1_1 + Gram', prepare=prepare)


def test_forward_two_launch_cover_every_seam_row():
    """362 x 362: conv1_2 and conv2_2 are covered by two launches of different tiles.  The spike runs down the first and the
    last column, so it visits every row - the seam's too, wherever the cost model put it."""
    h, w = COVER
    forward_sweep(COVER, 'max', [(y, x) for y in range(h) for x in (0, w - 1)], 'forward 362x362 two-launch cover')


# ---- backward --------------------------------------------------------------------------------------------------------------
def oracle_maps(image, last_layer, pooling='max', decisions=None):
    """{tap: float64 map} up to ``last_layer`` (the image requires grad: the maps are autograd nodes)."""
    layers = [t for t in TAPS if t <= last_layer]
    return O.vgg_features(image, centre_weights64(), layers, pooling, decisions)


def oracle_gradients(image, seeds, decisions):
    """{tap: float64 gradient of sum_t <cotangent_t, tap_t> with respect to the tap, times the tap's ReLU mask} - the form a data
    gradient stages - for every tap up to the deepest seeded one, on the branches ``decisions``."""
    top = max(seeds)
    img = image.double().requires_grad_(True)
    feats = oracle_maps(img, top, 'max', decisions)
    total = 0
    for t in TAPS:
        if t <= top:
            feats[t].retain_grad()
        if t in seeds:
            total = total + (feats[t] * seeds[t].double()).sum()
    total.backward()
    return {t: (feats[t].grad * decisions[t] if t in RELUS else feats[t].grad).detach() for t in TAPS if t <= top}


def dominance(tensor, y, x):
    """max |T| at pixel (y, x) over max |T| at every other pixel."""
    m = tensor[0].abs().amax(0)
    at = float(m[y, x])
    m = m.clone()
    m[y, x] = 0
    return at / max(float(m.max()), 1e-300)


def cotangent(plan_shapes, tap, q, scale=1.0):
    """A seeded cotangent in +-0.5 with the spike AMP at pixel q of every channel."""
    c, h, w = plan_shapes[tap]
    g = torch.Generator().manual_seed(1000 + tap)
    cot = torch.rand((1, c, h, w), generator=g) - 0.5
    cot[0, :, q[0], q[1]] = AMP
    return (cot * scale).contiguous()


def tap_shapes(size):
    h, w = size
    out = {}
    for t in TAPS:
        c = 64 if t < 5 else 128 if t < 10 else 256 if t < 19 else 512
        out[t] = (c, h >> LEVEL[t], w >> LEVEL[t])
    return out


def edge_positions(h, w):
    """The four corners, the last row and the last column of an h x w map."""
    return sorted({(0, 0), (0, w - 1)} | {(h - 1, x) for x in range(w)} | {(y, w - 1) for y in range(h)})


def g_failures(words, grads, where, slack, tau=TAU, exempt=()):
    """Words 16 .. 28 and 32 .. 35 against ``grads`` ({tap: max |masked gradient|}); a word shared by a pool and the
    convolution that feeds it covers both; a word none of the taps uses reads 0."""
    out = []
    for word in G_WORDS:
        ms = [grads[t] for t in TAPS if G_WORD[t] == word and t in grads]
        if not ms:
            out += zero_failures(words, [word], where)
            continue
        taps = [t for t in TAPS if G_WORD[t] == word and t in grads]
        out += bound_failures(f'{where} g word {word} (features{taps})', words[word], max(ms), tau, loose=word not in exempt)
        slack.see(word, words[word], max(ms), exempt=word in exempt)
    return out


BACKWARD_CASES = {'relu1_1': [1], 'relu3_1': [11], 'pool4': [27], 'relu5_1': [29], 'all four': [1, 11, 27, 29]}


@pytest.mark.parametrize('case', list(BACKWARD_CASES))
def test_backward_spike_cotangents(case):
    """Plan.forward then Plan.backward with a spike cotangent at one tap (relu1_1, relu3_1, pool 4, relu5_1) or at all four,
    the spike on the four corners, the last row and the last column of the (deepest) tap; the forward spike sits at the same
    place, so that every ReLU on the way down is open.  Words 16 .. 28 and 32 .. 35 against the float64 intermediate gradients
    on the plan's own branches; then a second backward over the same forward with cotangents 4096 x smaller: every g word must be
    that pass's own."""
    layers = BACKWARD_CASES[case]
    top, level = max(layers), LEVEL[max(layers)]
    shapes = tap_shapes(SIZE)
    base = base_image(SIZE)
    positions = edge_positions(*shapes[top][1:])
    torch.set_num_threads(min(16, torch.get_num_threads()))

    def inputs(q):
        p = (q[0] << level, q[1] << level)
        seeds = {t: cotangent(shapes, t, (p[0] >> LEVEL[t], p[1] >> LEVEL[t])) for t in layers}
        return p, spiked(base, *p), seeds

    def dominated(grads, p, where):
        for t, g in grads.items():
            d = dominance(g, p[0] >> LEVEL[t], p[1] >> LEVEL[t])
            assert d >= DOMINANCE, f'{where}: the spike is only {d:.2f} x the rest of features[{t}]\'s gradient: tune the inputs'

    # CPU first, on float64's own branches: the spike dominates every bounded gradient at the corners
    for q in [(0, 0), (0, shapes[top][2] - 1), (shapes[top][1] - 1, 0), (shapes[top][1] - 1, shapes[top][2] - 1)]:
        p, img, seeds = inputs(q)
        with torch.no_grad():
            maps = oracle_maps(img.double(), top)
        dominated(oracle_gradients(img, seeds, O.decisions_from_maps({t: maps[t] for t in RELUS if t <= top})), p, f'{case} {q}')

    net, plan = make_plan(SIZE)
    slack, failures = Slack(f'backward {case}'), []
    unused = NEVER_USED + list(HEAD_WORDS)
    for q in positions:
        p, img, seeds = inputs(q)
        plan.forward(img.to(DEV), 29)
        torch.cuda.synchronize()
        decisions = O.decisions_from_maps({t: plan.feature(t).cpu() for t in RELUS if t <= top})
        grads = oracle_gradients(img, seeds, decisions)
        dominated(grads, p, f'{case} {q} (plan\'s branches)')
        m = {t: float(g.abs().max()) for t, g in grads.items()}
        for scale in (1.0, 1.0 / 4096):
            plan.backward(layers, [(seeds[t] * scale).to(DEV) for t in layers])
            words = plan.debug_read(2, 64).tolist()
            where = f'backward {case} tap pixel {q}' + (' / 4096' if scale != 1.0 else '')
            failures += g_failures(words, {t: v * scale for t, v in m.items()}, where, slack)
            failures += zero_failures(words, unused, where)
    slack.report()
    print(f'[bounds] backward {case}: {len(positions)} spike positions x 2 passes, {len(failures)} failures')
    assert_none(failures, f'backward {case}')


# ---- closures --------------------------------------------------------------------------------------------------------------
def ramp_mask(h, w):
    """m[y, x] = clamp(2 (x / (W - 1) - 0.25), 0, 1) (0.5 + 0.5 y / (H - 1)): a quarter exact zeros, a band of exact ones."""
    x = torch.arange(w, dtype=torch.float64) / (w - 1)
    y = torch.arange(h, dtype=torch.float64) / (h - 1)
    return ((2 * (x - 0.25)).clamp(0, 1)[None, :] * (0.5 + 0.5 * y)[:, None]).float().contiguous()


def _own_targets(plan, target, regions=1):
    """Content and style targets from the plan's own forward of ``target`` (what the targets are does not matter here)."""
    plan.forward(target, 29)
    plan.set_content_target_from_forward()
    for j, layer in enumerate(plan.style_layers):
        mean, srm = plan.moments(layer)
        for r in range(regions):
            if regions > 1:
                plan.set_region_style_target(r, j, mean, srm)
            else:
                plan.set_style_target(j, mean, srm)


def _configure(plan, config, size, target):
    if config == 'taps':
        plan.set_taps([13, 18], [3, 9, 20, 24])          # relu and pool taps, a layer that feeds a pool, nothing above relu4_3
    elif config == 'gram':
        plan.set_loss_kinds('mse', 'gram')
    elif config == 'mask':
        plan.set_style_mask(ramp_mask(*size).to(DEV))
    elif config == 'regions':
        ramp = ramp_mask(*size)
        plan.set_style_regions([ramp.to(DEV), (1 - ramp).contiguous().to(DEV)])
    _own_targets(plan, target, 2 if config == 'regions' else 1)


CLOSURES = [('default', SIZE, {}), ('default', ALIGNED, {}), ('default', ALIGNED, dict(ST_CONV_FAT=2)), ('taps', SIZE, {}),
            ('gram', SIZE, {}), ('mask', SIZE, {}), ('regions', SIZE, {})]


@pytest.mark.parametrize('config,size,opts', CLOSURES, ids=[f'{c}-{s[0]}x{s[1]}' + ('-' + _opts_id(o) if o else '') for c, s, o in CLOSURES])
def test_closure_bounds(config, size, opts):
    """loss_and_grad with targets from a second image and the forward spike on three corners of the coarsest level: both
    halves on every word the configuration uses, every other word 0.  The y words against the float64 oracle (the default
    closure's argmax-coded forward leaves no map of relu1_2, 2_2, 3_4, 4_4 - at 76 x 128 the first two are coded, and with
    the fat tile forced every pooled layer's epilogue writes pool and codes) and against the device's maps where the pass
    writes them; the g words against the gradient maps the pass left (``debug_read(16 + i)``), exactly."""
    h, w = size
    ys, xs = ((h >> 4) - 1) << 4, ((w >> 4) - 1) << 4
    positions = [(0, xs), (ys, 0), (ys, xs)]
    base = base_image(size)
    general = config != 'default'
    top = 24 if config == 'taps' else 29
    torch.set_num_threads(min(16, torch.get_num_threads()))
    # CPU first: the float64 maps of the three spiked images, and the spike's dominance in each
    reference = []
    for y, x in positions:
        with torch.no_grad():
            maps = oracle_maps(spiked(base, y, x).double(), top)
        for t in RELUS:
            if t <= top:
                d = dominance(maps[t], y >> LEVEL[t], x >> LEVEL[t])
                assert d >= DOMINANCE, f'spike ({y}, {x}): only {d:.2f} x the rest of features[{t}]: tune the inputs'
        reference.append({t: float(maps[t].abs().max()) for t in RELUS if t <= top})

    name = f'{"general" if general else "default"} closure'
    exempt = LOOSE_EXEMPT[name]
    shapes = tap_shapes(size)
    coded = () if general else tuple(t - 1 for t in POOLS)         # (their maps may be argmax codes: the oracle alone)
    with _hip().options(**opts):
        net, plan = make_plan(size)
        _configure(plan, config, size, base_image(size, 92).to(DEV))
        n_style = len(plan.style_layers)
        slack, failures = Slack(f'{config} closure {h}x{w} {_opts_id(opts)}'), []
        for (y, x), ref in zip(positions, reference):
            where = f'{config} closure spike ({y}, {x})'
            plan.loss_and_grad(spiked(base, y, x).to(DEV))
            words, bad = forward_failures(plan, 'max', top, where, slack, y_reference=ref, skip_device=coded)
            failures += bad
            grads = {}
            for i, t in enumerate(TAPS):
                if t <= top:
                    grads[t] = float(plan.debug_read(16 + i, shapes[t][0] * shapes[t][1] * shapes[t][2]).abs().max())
            failures += g_failures(words, grads, where, slack, tau=0.0, exempt=exempt)
            failures += zero_failures(words, NEVER_USED + [wd for wd in HEAD_WORDS if wd >= 48 + n_style], where)
            for j in range(n_style):                                # a listed head's word: set, finite (its matrix is not readable)
                if not (math.isfinite(words[48 + j]) and words[48 + j] > 0):
                    failures.append(f'{where} head word {48 + j}: {words[48 + j]!r}')
    slack.report()
    assert_none(failures, f'{config} closure {h}x{w}')


# ---- the hand-over through a step ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['adam', 'adam-tail-1', 'adam-tail-0', 'lbfgs'])
def test_bounds_after_a_step_are_a_fresh_forwards(mode):
    """loss_and_grad, then one step (st_plan_step - with the update folded into conv1_1's fold kernel, ST_STEP_TAIL=2, with
    the update kernel clearing the words, 1, and with nothing clearing them, 0 - or st_plan_lbfgs_step), then Plan.forward: all
    64 words are those of a fresh plan's forward of the same image.  The step's tail clears the words and tells the next forward
    to skip its own clearing (st_plan::amax_clean); a word the hand-over misses would still hold the closure's bound."""
    hip = _hip()
    size = SIZE
    base, other = base_image(size).to(DEV), spiked(base_image(size, 93), 48, 80).to(DEV)
    net, plan = make_plan(size)
    _own_targets(plan, base_image(size, 92).to(DEV))
    opts = {'adam-tail-1': dict(ST_STEP_TAIL=1), 'adam-tail-0': dict(ST_STEP_TAIL=0)}.get(mode, {})
    with hip.options(**opts):
        plan.loss_and_grad(spiked(base, 0, 0, AMP * 64))         # large bounds everywhere: a stale one shows
        x = base.clone()
        ema = torch.zeros_like(x)
        if mode == 'lbfgs':
            hip.LBFGS(x).step(plan, x, ema, 0.99)
        else:
            plan.step(x, torch.zeros_like(x), torch.zeros_like(x), ema, 1, 0.02)
        after_step = plan.debug_read(2, 64).tolist()
        plan.forward(other, 29)
        got = plan.debug_read(2, 64).tolist()
    net2, fresh = make_plan(size)
    fresh.forward(other, 29)
    want = fresh.debug_read(2, 64).tolist()
    print(f'[bounds] hand-over {mode}: words set after the step {[w for w in range(64) if after_step[w] != 0]}')
    assert all(math.isfinite(v) and v >= 0 for v in got + want)
    bad = [(w, got[w], want[w]) for w in range(64) if limit(got[w]) != limit(want[w])]
    assert not bad, f'hand-over {mode}: (word, after the step, fresh plan) {bad}'
    assert [w for w in range(64) if want[w] != 0] == list(range(13))
