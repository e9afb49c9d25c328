"""Scenes for the single-time-effect kernel (csrc/ste.hip) and a numpy emulation of its tile
algorithm, shared by test_cpu_ste.py (which proves on the CPU what each scene is sensitive to)
and test_gpu_ste.py (which runs the scenes on the device).

The kernel keeps a 128 x 64 tile in registers over the `st` <= 8 steps of a launch and writes the
pixels at least `st` from the tile border.  Three things can go wrong there without a random
scene noticing: the halo (a dependency chain of st pixels must cross a tile border), the exchange
of a wave's first and last row with the waves above and below (LDS, alternating slot), and the
carry between the two 64-bit ballot words of a row.  The scenes here are built for them:

fuse scenes       all zeros, a constant threshold of 16.  A fuse of length S ends on pixel P and
                  runs along a direction u: in step k of a launch the pixel A(k) = P - (S-1-k) u
                  gets 1000 and, for k > 0, A(k-1) gets 20 - above the threshold only if A(k-1)
                  did not absorb its 1000 the step before, which it does exactly when it was a
                  single pixel.  'lit': A(-1) gets 1000 in step 0, so A(0) is half of a pair, is
                  not absorbed, and the pair walks to P.  'unlit': nothing on A(-1); every A(k)
                  is a single pixel and P is clean.  'soft': A(-1) gets 20 in step 0 (lights the
                  fuse while its average is 0) and 1000 alone in the last step (absorbed): a
                  launch that reads A(-1)'s state after its neighbour has written it sees no
                  light.  P is the first or last output pixel of a tile in x or y, u points into
                  the tile, S is the launch's step count: A(-1) lies on the outermost ring of the
                  tile that owns P.
adjacency scenes  pairs of candidates in all eight neighbour directions across every wave row
                  boundary of a tile, the 63 | 64 column seam, the output-tile borders and the
                  image's edges and corners, in step 0 and step 1 of a launch.
"""
import numpy as np

TILE_W, TILE_H, WAVE_ROWS, MAX_STEPS = 128, 64, 8, 8
NLF_CONST, NSTD_CONST, THR_CONST = (4.0, 0.0, 0.0), 4, 16.0
BRIGHT, PROBE = 1000, 20

NLF = (3.0, 150.0, 1.1)
NLF8 = (1.0, 20.0, 0.4)   # for uint8 frames (the random scene / 8)


def random_scene(n, h, w, dtype, seed, nan=True):
    """the random scene of the first STE tests: 1 % hits, horizontal pairs"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    base = 200 + 1500 * (x + y) / max(h + w - 2, 1)
    f = base + 6 * rng.standard_normal((n, h, w))
    f += (rng.random((n, h, w)) < 0.01) * 600                      # hits
    f += (rng.random((n, h, w)) < 0.04) * rng.uniform(20, 60, (n, h, w))   # near the threshold
    for k in range(n):                                              # pairs, so that some survive
        ys, xs = rng.integers(0, h, 8), rng.integers(0, w, 8)
        f[k, ys, xs] += 700
        f[k, ys, np.minimum(xs + 1, w - 1)] += 700
    if dtype == np.uint8:
        f = f / 8
    if np.dtype(dtype).kind == 'f':
        if nan:
            f[rng.random((n, h, w)) < 0.002] = np.nan
        return f.astype(dtype)
    return np.clip(np.round(f), 0, np.iinfo(dtype).max).astype(dtype)


def split_steps(steps, per_launch=MAX_STEPS):
    """steps of the launches of one ipa_ste_dev call"""
    out = []
    while steps > 0:
        out.append(min(per_launch, steps))
        steps -= out[-1]
    return out


def _tiles(h, w, halo):
    """(by, bx, y0, x0) of a launch's workgroups: tile origin, halo included"""
    oy, ox = TILE_H - 2 * halo, TILE_W - 2 * halo
    for by in range(-(-h // oy)):
        for bx in range(-(-w // ox)):
            yield by, bx, by * oy - halo, bx * ox - halo


# ------------------------------------------------------------------ fuse scenes ----
KINDS = ('lit', 'unlit', 'soft')
# directions (dy, dx) that point into the tile from each end
INBOUND = {'x0': ((0, 1), (1, 1), (-1, 1)), 'x1': ((0, -1), (1, -1), (-1, -1)),
           'y0': ((1, 0), (1, 1), (1, -1)), 'y1': ((-1, 0), (-1, 1), (-1, -1))}


def _grow(m):
    p = np.zeros((m.shape[0] + 2, m.shape[1] + 2), bool)
    p[1:-1, 1:-1] = m
    out = np.zeros_like(m)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + m.shape[0], dx:dx + m.shape[1]]
    return out


def fuse_scene(launches, h, w):
    """-> (step frames float64 (sum(launches), h, w), fuses).  A fuse is a dict: launch, S, end,
    u, kind, P, px (the pixels A(-1) ... A(S-1)).  Fuses of one launch are at least two pixels
    apart; no fuse touches a pixel that absorbed something in an earlier launch."""
    g = np.zeros((sum(launches), h, w))
    dirty = np.zeros((h, w), bool)
    fuses, done = [], 0
    for li, st in enumerate(launches):
        busy = np.zeros((h, w), bool)
        # the tiling of the launch, and the one a kernel with a halo of st - 1 would use: there a
        # chain of st pixels that ends on a tile's first output pixel starts outside the tile
        for halo, by, bx, y0, x0 in [(hl,) + t for hl in (st, st - 1) for t in _tiles(h, w, hl)]:
            oy, ox = TILE_H - 2 * halo, TILE_W - 2 * halo
            ya, yb = y0 + halo, min(y0 + halo + oy, h) - 1   # first / last output pixel
            xa, xb = x0 + halo, min(x0 + halo + ox, w) - 1
            for ei, end in enumerate(('x0', 'x1', 'y0', 'y1')):
                for ui, u in enumerate(INBOUND[end]):
                    kind = KINDS[(by + bx + ei + ui + li) % 3]
                    if kind == 'soft' and st < 3:
                        kind = 'lit'
                    # P on the end's line, somewhere along it
                    span = range(ya + 1, yb) if end[0] == 'x' else range(xa + 1, xb)
                    for c in span:
                        P = {'x0': (c, xa), 'x1': (c, xb), 'y0': (ya, c), 'y1': (yb, c)}[end]
                        px = [(P[0] - (st - 1 - j) * u[0], P[1] - (st - 1 - j) * u[1])
                              for j in range(-1, st)]
                        if not all(0 <= y < h and 0 <= x < w for y, x in px):
                            continue
                        # the chain stays in the rows / columns of P's tile along the end's line
                        if not all((ya <= y <= yb) if end[0] == 'x' else (xa <= x <= xb)
                                   for y, x in px):
                            continue
                        ys, xs = zip(*px)
                        if busy[ys, xs].any() or dirty[ys, xs].any():
                            continue
                        m = np.zeros((h, w), bool)
                        m[ys, xs] = True
                        busy |= _grow(_grow(m))
                        for k in range(st):
                            g[done + k][px[k + 1]] = BRIGHT
                            if k > 0:
                                g[done + k][px[k]] = PROBE
                        if kind == 'lit':
                            g[done][px[0]] = BRIGHT
                        elif kind == 'soft':
                            g[done][px[0]] = PROBE
                            g[done + st - 1][px[0]] = BRIGHT
                        if kind != 'lit':
                            dirty[ys, xs] = True
                        fuses.append(dict(launch=li, S=st, end=end, u=u, kind=kind, P=P, px=px,
                                          last_step=done + st - 1,
                                          tiling='exact' if halo == st else 'short'))
                        break
        done += st
    return g, fuses


def fuse_frames(launches, h, w, dtype):
    """frames of a constructor call: a zero frame, then the step frames (the first pair's minimum
    is 0, its maximum the first step frame)"""
    g, fuses = fuse_scene(launches, h, w)
    return np.concatenate([np.zeros((1, h, w)), g]).astype(dtype), fuses


def link_mask(fuses, h, w):
    """a caller mask that forbids one link, A(0), of every second unlit fuse of two or more steps
    to absorb anything: it stays a candidate and lights the fuse from there"""
    m = np.ones((h, w), bool)
    hit = []
    for i, f in enumerate(fuses):
        if f['kind'] == 'unlit' and f['S'] >= 2 and i % 2 == 0:
            m[f['px'][1]] = False
            hit.append(f)
    return m, hit


# ------------------------------------------------------------------ adjacency scenes ----
DIRS8 = tuple((dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx)


def adjacency_scene(st, h, w, amp):
    """-> (step frames float64 (st, h, w), pairs).  A pair is (step, class, a, b, u): pixels a and
    b = a + u get `amp` in that step and nothing else touches them.  Pairs are laid in step 0 and,
    where the launch has one, step 1."""
    g = np.zeros((st, h, w))
    pairs = []
    oy, ox = TILE_H - 2 * st, TILE_W - 2 * st
    for step in range(min(st, 2)):
        busy = np.zeros((h, w), bool)
        want = []
        # wave row boundaries of tile (1, 0): tile rows r | r + 1
        y0 = oy - st
        for r in range(WAVE_ROWS - 1, TILE_H - 1, WAVE_ROWS):
            for dx in (-1, 0, 1):
                want.append(('wave %d|%d' % (r, r + 1), (y0 + r, None), (1, dx), 'x'))
        # the column seam of tile (., 0): tile columns 63 | 64
        for dy in (-1, 0, 1):
            want.append(('seam', (None, 63 - st), (dy, 1), 'y'))
        # output-tile borders
        for d in (-1, 0, 1):
            want.append(('tile x', (None, ox - 1), (d, 1), 'y'))
            want.append(('tile y', (oy - 1, None), (1, d), 'x'))
        # image edges: along the edge and away from it
        for u in ((0, 1), (1, 0), (1, 1), (1, -1)):
            want.append(('top', (0, None), u, 'x'))
            want.append(('bottom', (h - 1 - u[0], None), u, 'x'))
            want.append(('left', (None, max(0, -u[1])), u, 'y'))
            want.append(('right', (None, w - 1 - max(0, u[1])), u, 'y'))
        for cls, (y, x), u, free in want:
            for c in range(3 + 17 * step, (w if free == 'x' else h) - 3):
                a = (y, c) if free == 'x' else (c, x)
                b = (a[0] + u[0], a[1] + u[1])
                if not (0 <= b[0] < h and 0 <= b[1] < w) or busy[a] or busy[b]:
                    continue
                m = np.zeros((h, w), bool)
                m[a] = m[b] = True
                busy |= _grow(_grow(m))
                g[step][a] = g[step][b] = amp
                pairs.append((step, cls, a, b, u))
                break
            else:
                raise AssertionError('no room for %s' % cls)
        # corners: the corner pixel and its diagonal neighbour (step 0), its two edge neighbours
        # (step 1)
        for cy, cx in ((0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)):
            sy, sx = (1 if cy == 0 else -1), (1 if cx == 0 else -1)
            bs = [(cy + sy, cx + sx)] if step == 0 else [(cy + sy, cx), (cy, cx + sx)]
            for b in bs:
                g[step][cy, cx] = g[step][b] = amp
                pairs.append((step, 'corner', (cy, cx), b, (b[0] - cy, b[1] - cx)))
    return g, pairs


def adjacency_frames(st, h, w, dtype):
    amp = 100
    g, pairs = adjacency_scene(st, h, w, amp)
    return np.concatenate([np.zeros((1, h, w)), g]).astype(dtype), pairs


# ------------------------------------------------------------------ the tile algorithm ----
def _tile_single_pixels(s, defect):
    """removeSinglePixels on a 64 x 128 tile, zeros beyond it, as the kernel's ballots do it"""
    hh, ww = s.shape
    p = np.zeros((hh + 2, ww + 2), bool)
    p[1:-1, 1:-1] = s
    rows = np.arange(hh) % WAVE_ROWS
    nb = np.zeros_like(s)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            if not (dy or dx):
                continue
            n = p[1 + dy:1 + dy + hh, 1 + dx:1 + dx + ww].copy()
            if defect == 'waves':            # the rows above and below a wave taken as empty
                if dy == -1:
                    n[rows == 0] = False
                if dy == 1:
                    n[rows == WAVE_ROWS - 1] = False
            if defect == 'seam':             # no carry between the two ballot words
                if dx == -1:
                    n[:, 64] = False
                if dx == 1:
                    n[:, 63] = False
            nb |= n
    return s & nb


class SteTiles(object):
    """SteNumpy's contract computed the way ste_kernel does: per launch of up to 8 steps and per
    128 x 64 tile a crop of the state, zeros beyond tile and image, removeSinglePixels per step
    within the tile, output rings from `halo` inwards.

    defect: None | 'waves' | 'seam' | 'inplace' (a launch reads the state from the buffer it
    writes, tiles in raster order) | ('halo', i) (launch i of the call - counted over the
    object's life - is placed with a halo one ring short; i = 'all': every launch)"""

    def __init__(self, frames, nlf, nstd, defect=None, per_launch=MAX_STEPS):
        from .test_cpu_ste import bounded_nlf
        f0 = np.asarray(frames[0]).astype(np.float64)
        f1 = np.asarray(frames[1])
        self.avg = np.min((f0, f1), axis=0)
        self.count = np.ones(self.avg.shape, dtype=np.int64)
        self.thr = bounded_nlf(self.avg, *nlf) * nstd
        self.mask_ste = np.zeros(self.avg.shape, dtype=bool)
        self.mask_clean = np.ones(self.avg.shape, dtype=bool)
        self.defect, self.per_launch, self.launch_no = defect, per_launch, 0
        steps = [np.max((f0, f1), axis=0)] + [np.asarray(f, np.float64) for f in frames[2:]]
        self.run(steps, first=True)

    def add(self, frames, mask=None):
        """one ipa_ste_dev call that continues the state over `frames`"""
        self.run([np.asarray(f, np.float64) for f in frames], mask=mask)
        return self

    def run(self, steps, mask=None, first=False):
        done = 0
        for st in split_steps(len(steps), self.per_launch):
            self._launch(steps[done:done + st], mask, first and done == 0)
            done += st

    def _launch(self, g, mask, first):
        st = len(g)
        h, w = self.avg.shape
        d = self.defect
        halo = st
        if isinstance(d, tuple) and d[0] == 'halo' and d[1] in ('all', self.launch_no):
            halo = st - 1
        self.launch_no += 1
        alias = d == 'inplace' and not first   # the first pair has no input state
        avg_in, cnt_in = self.avg, self.count
        avg_out = avg_in if alias else avg_in.copy()
        cnt_out = cnt_in if alias else cnt_in.copy()
        clean_out = np.ones((h, w), bool)
        rsp_defect = d if d in ('waves', 'seam') else None
        for by, bx, y0, x0 in _tiles(h, w, halo):
            ys, xs = np.arange(y0, y0 + TILE_H), np.arange(x0, x0 + TILE_W)
            inside = ((ys >= 0) & (ys < h))[:, None] & ((xs >= 0) & (xs < w))[None, :]
            yc, xc = np.clip(ys, 0, h - 1)[:, None], np.clip(xs, 0, w - 1)[None, :]
            avg, cnt, thr = avg_in[yc, xc].copy(), cnt_in[yc, xc].copy(), self.thr[yc, xc]
            keep = np.ones_like(inside) if mask is None else np.asarray(mask, bool)[yc, xc]
            ste = np.zeros_like(inside)
            for gk in g:
                gv = gk[yc, xc]
                with np.errstate(invalid='ignore'):
                    s = inside & (gv - avg > thr)
                sp = _tile_single_pixels(s, rsp_defect)
                ste |= sp
                last = ~sp
                take = last & keep
                cnt[take] += 1
                avg[take] = avg[take] + (gv[take] - avg[take]) / cnt[take]
            out = inside.copy()
            out[:halo] = out[TILE_H - halo:] = False
            out[:, :halo] = out[:, TILE_W - halo:] = False
            oy, ox = np.nonzero(out)
            gy, gx = ys[oy], xs[ox]
            avg_out[gy, gx] = avg[oy, ox]
            cnt_out[gy, gx] = cnt[oy, ox]
            self.mask_ste[gy, gx] |= ste[oy, ox]
            clean_out[gy, gx] = last[oy, ox]
        self.avg, self.count, self.mask_clean = avg_out, cnt_out, clean_out


def same_state(a, b):
    """avg bits, count, both masks of two SteNumpy / SteTiles"""
    from .test_cpu_ste import same_f64
    return bool(same_f64(a.avg, b.avg) and np.array_equal(a.count, b.count) and
                np.array_equal(a.mask_ste, b.mask_ste) and np.array_equal(a.mask_clean, b.mask_clean))


# ------------------------------------------------------------------ the case table ----
FUSE_HW, ADJ_HW = (150, 260), (130, 140)
FUSE_STEPS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17)   # n - 1 of a constructor call
CONT_MORE = (3, 8, 9, 12, 17)                        # frames of a continuing ops.ste_update call
ADJ_STEPS = (1, 2, 8)
ADJ_DTYPES = (np.uint8, np.uint16, np.float32, np.float64)
_cache = {}


def _once(key, make):
    if key not in _cache:
        _cache[key] = make()
        for a in _cache[key]:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return _cache[key]


def fuse_case(steps):
    """-> (float32 frames, fuses, SteNumpy) of a constructor call over steps + 1 frames"""
    from .test_cpu_ste import SteNumpy

    def make():
        fr, fuses = fuse_frames(split_steps(steps), FUSE_HW[0], FUSE_HW[1], np.float32)
        return fr, fuses, SteNumpy(fr, NLF_CONST, NSTD_CONST)
    return _once(('fuse', steps), make)


def cont_case(n_more):
    """-> (uint16 frames, fuses, caller mask, SteNumpy): the first pair in one call, then n_more
    frames under a caller mask in a second one"""
    from .test_cpu_ste import SteNumpy

    def make():
        fr, fuses = fuse_frames([1] + split_steps(n_more), FUSE_HW[0], FUSE_HW[1], np.uint16)
        m, hit = link_mask([f for f in fuses if f['launch'] > 0], *FUSE_HW)
        ref = SteNumpy(fr[:2], NLF_CONST, NSTD_CONST)
        for f in fr[2:]:
            ref.add(f, m)
        return fr, fuses, m, ref, hit
    return _once(('cont', n_more), make)


def adj_case(st, dtype):
    from .test_cpu_ste import SteNumpy

    def make():
        fr, pairs = adjacency_frames(st, ADJ_HW[0], ADJ_HW[1], dtype)
        return fr, pairs, SteNumpy(fr, NLF_CONST, NSTD_CONST)
    return _once(('adj', st, np.dtype(dtype).name), make)
