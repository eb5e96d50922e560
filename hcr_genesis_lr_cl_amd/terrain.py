"""Heightfield generation (int16 grid + per-tile env origins): on the host with numpy, or -- `Terrain(cfg, device="cuda:0")`, what
HipSimulator uses -- on the device by one init-time kernel (include/lgsim.h lg_terrain_generate) that evaluates every pixel of every
tile from a descriptor table; the numpy draws the reference takes (np.random.choice / randint call order) are taken here on the host and
injected.  Both reproduce the reference grid sample for sample.

Restates the heightfield path of the reference's terrain generator (legged_gym/utils/terrain.py:37-203): the randomized, curriculum
and selected modes, and all eight heightfield sub-terrain generators of legged_gym/utils/terrain_utils.py -- random uniform (:34-96),
pyramid slope (:128-181), discrete obstacles (:204-258), wave (:273-303), pyramid stairs (:330-372), stepping stones (:391-469), gap
(:471-497) and pit (:499-519).  With the same `np.random.seed` it reproduces the reference grid sample for sample and leaves numpy's
generator in the same state (tests/test_terrain.py, tests/test_terrain_kinds.py against tests/golden/terrain_*.npz).

Grid convention: `height_field_raw[ix, iy]`, x = rows (terrain levels / difficulty), y = cols
(terrain types); world x = ix * horizontal_scale - border_size; height = value * vertical_scale.
Sub-terrain tiles are square (the reference builds them width x width), so the generators' x and y extents coincide.
Trimesh terrain and the mesh_* generators are not provided (genesis_simulator.py:271 raises for trimesh as well).
"""
from __future__ import annotations

import numpy as np
from scipy import interpolate


class _Tile:
    def __init__(self, n, vscale, hscale):
        self.width = self.length = n
        self.vertical_scale, self.horizontal_scale = vscale, hscale
        self.height_field_raw = np.zeros((n, n), dtype=np.int16)


def _span(a, b, n):
    """numpy's reading of the slice [a:b] on an axis of length n (negative bounds count from the end), as a half-open [lo, hi)."""
    lo, hi, _ = slice(a, b).indices(n)
    return lo, max(lo, hi)


# ---- the reference's draws and integer parameters, shared by the host generators and the device descriptors ---------------------------
def _uniform_spline(t, min_height, max_height, step, downsampled_scale):
    """terrain_utils.py:57-87: the coarse random grid (one np.random.choice) and its degree-1 spline; returns what the up-sampling
    evaluates."""
    if downsampled_scale is None:
        downsampled_scale = t.horizontal_scale
    edge = int(0.2 / t.horizontal_scale)
    lo, hi, step = int(min_height / t.vertical_scale), int(max_height / t.vertical_scale), int(step / t.vertical_scale)
    levels = np.arange(lo, hi + step, step)
    shape = (int((t.width - 2 * edge) * t.horizontal_scale / downsampled_scale), int((t.length - 2 * edge) * t.horizontal_scale / downsampled_scale))
    coarse_h = np.random.choice(levels, shape)
    a, bx, by = edge * t.horizontal_scale, (t.width - edge) * t.horizontal_scale, (t.length - edge) * t.horizontal_scale
    spline = interpolate.RectBivariateSpline(np.linspace(a, by, shape[1]), np.linspace(a, bx, shape[0]), coarse_h, kx=1, ky=1)
    return edge, spline, np.linspace(a, by, t.length - 2 * edge), np.linspace(a, bx, t.width - 2 * edge)


def _obstacle_rects(t, max_height, min_size, max_size, num_rects):
    """terrain_utils.py:225-243: (i0, j0, w, l, height) per rectangle, in draw order (same np.random.choice call order)."""
    mh = int(max_height / t.vertical_scale)
    smin, smax = int(min_size / t.horizontal_scale), int(max_size / t.horizontal_scale)
    ni, nj = t.height_field_raw.shape
    heights = [-mh, -mh // 2, mh // 2, mh]
    sizes = range(smin, smax, 4)
    rects = []
    for _ in range(num_rects):
        w = np.random.choice(sizes)
        l = np.random.choice(sizes)
        i0 = np.random.choice(range(0, ni - w, 4))
        j0 = np.random.choice(range(0, nj - l, 4))
        rects.append((int(i0), int(j0), int(w), int(l), int(np.random.choice(heights))))
    return rects


def _stone_rects(t, stone_size, stone_distance, max_height, platform_size, depth):
    """terrain_utils.py:408-455 (the `length >= width` branch: tiles are square): background, rectangles (i0, j0, w, l, height) in
    draw order and the platform span.  Every draw of the reference is taken, the per-row np.random.randint and the "fill first hole"
    np.random.choice included, also when that hole is empty (its rectangle then has w = 0)."""
    W, L = t.width, t.length
    ss, sd = int(stone_size / t.horizontal_scale), int(stone_distance / t.horizontal_scale)
    mh, plat = int(max_height / t.vertical_scale), int(platform_size / t.horizontal_scale)
    if ss + sd <= 0:
        raise ValueError("stepping_stones_terrain: stone_size + stone_distance is below one pixel (the reference loops forever)")
    heights = np.arange(-mh - 1, mh, step=1)
    rects, start_y = [], 0
    while start_y < L:
        stop_y = min(L, start_y + ss)
        start_x = np.random.randint(0, ss)
        rects.append((0, start_y, max(0, start_x - sd), stop_y - start_y, int(np.random.choice(heights))))    # fill first hole
        while start_x < W:
            stop_x = min(W, start_x + ss)
            rects.append((start_x, start_y, stop_x - start_x, stop_y - start_y, int(np.random.choice(heights))))
            start_x += ss + sd
        start_y += ss + sd
    return int(depth / t.vertical_scale), rects, _span((W - plat) // 2, (W + plat) // 2, W)


def _gap_spans(t, gap_size, platform_size):
    """terrain_utils.py:478-490: the -1000 square and the zero platform square inside it, as spans of numpy's slices."""
    gs, plat = int(gap_size / t.horizontal_scale), int(platform_size / t.horizontal_scale)
    c, x1 = t.length // 2, plat // 2
    return _span(c - (x1 + gs), c + (x1 + gs), t.width), _span(c - x1, c + x1, t.width)


def _pit_span(t, depth, platform_size):
    """terrain_utils.py:503-509: the sunk square and its height."""
    half = int(platform_size / t.horizontal_scale / 2)
    return _span(t.length // 2 - half, t.length // 2 + half, t.width), -int(depth / t.vertical_scale)


def _wave_rows(t, num_waves, amplitude):
    """terrain_utils.py:292-301 up to the sum: edge, amplitude * cos(y / div) (1, n) and amplitude * sin(x / div) (n, 1), float64 with
    numpy's own cos / sin; None when num_waves <= 0 (the tile stays flat)."""
    amp = int(0.5 * amplitude / t.vertical_scale)
    edge = int(0.2 / t.horizontal_scale)
    if not num_waves > 0:
        return edge, None, None
    div = t.length / (num_waves * np.pi * 2)
    xx, yy = np.meshgrid(np.arange(edge, t.width - edge), np.arange(edge, t.length - edge), sparse=True)
    xx = xx.reshape(t.width - 2 * edge, 1)
    yy = yy.reshape(1, t.length - 2 * edge)
    return edge, amp * np.cos(yy / div), amp * np.sin(xx / div)


def _check_stairs(t, step_width):
    if int(step_width / t.horizontal_scale) < 1:
        raise ValueError("pyramid_stairs_terrain: step_width is below one pixel (the reference loops forever)")


# ---- host generators: the reference's signatures (selected mode passes the user's kwargs) -----------------------------------------------
def _pyramid_slope(t, slope=1, platform_size=1.):
    """terrain_utils.py:128-181."""
    edge = int(0.2 / t.horizontal_scale)
    n = t.width - 2 * edge
    c = int(t.width / 2)
    ramp = (c - np.abs(c - np.arange(edge, t.width - edge))) / c
    peak = int(slope * (t.horizontal_scale / t.vertical_scale) * (n / 2))
    t.height_field_raw[edge:-edge, edge:-edge] += (peak * ramp.reshape(n, 1) * ramp.reshape(1, n)).astype(np.int16)
    half = int(platform_size / t.horizontal_scale / 2)
    ref = t.height_field_raw[t.width // 2 - half, t.length // 2 - half]
    t.height_field_raw = np.clip(t.height_field_raw, min(ref, 0), max(ref, 0))


def _random_uniform(t, min_height, max_height, step=1, downsampled_scale=None):
    """terrain_utils.py:34-96 (coarse random grid, bilinear up-sampling, rounded)."""
    edge, spline, xs, ys = _uniform_spline(t, min_height, max_height, step, downsampled_scale)
    t.height_field_raw[edge:-edge, edge:-edge] += np.rint(spline(xs, ys)).astype(np.int16)


def _pyramid_stairs(t, step_width, step_height, platform_size=1.):
    """terrain_utils.py:330-372 (negative step height = descending pyramid)."""
    _check_stairs(t, step_width)
    w, h, plat = int(step_width / t.horizontal_scale), int(step_height / t.vertical_scale), int(platform_size / t.horizontal_scale)
    lo, hi, level = 0, t.width, 0
    while hi - lo > plat:
        t.height_field_raw[lo:hi, lo:hi] = level
        lo, hi, level = lo + w, hi - w, level + h


def _discrete_obstacles(t, max_height, min_size, max_size, num_rects, platform_size=1.):
    """terrain_utils.py:204-258 (same np.random.choice call order)."""
    for i0, j0, w, l, h in _obstacle_rects(t, max_height, min_size, max_size, num_rects):
        t.height_field_raw[i0:i0 + w, j0:j0 + l] = h
    plat = int(platform_size / t.horizontal_scale)
    a, b = (t.width - plat) // 2, (t.width + plat) // 2
    t.height_field_raw[a:b, a:b] = 0


def _wave(t, num_waves=1, amplitude=1.):
    """terrain_utils.py:273-303."""
    edge, cy, sx = _wave_rows(t, num_waves, amplitude)
    if cy is not None:
        t.height_field_raw[edge:t.width - edge, edge:t.length - edge] += (cy + sx).astype(t.height_field_raw.dtype)


def _stepping_stones(t, stone_size, stone_distance, max_height, platform_size=1., depth=-10):
    """terrain_utils.py:391-469."""
    bg, rects, (a, b) = _stone_rects(t, stone_size, stone_distance, max_height, platform_size, depth)
    t.height_field_raw[:, :] = bg
    for i0, j0, w, l, h in rects:
        t.height_field_raw[i0:i0 + w, j0:j0 + l] = h
    t.height_field_raw[a:b, a:b] = 0


def _gap(t, gap_size, platform_size=1.):
    """terrain_utils.py:471-497."""
    (a, b), (c, d) = _gap_spans(t, gap_size, platform_size)
    t.height_field_raw[a:b, a:b] = -1000
    t.height_field_raw[c:d, c:d] = 0


def _pit(t, depth, platform_size=1.):
    """terrain_utils.py:499-519."""
    (a, b), h = _pit_span(t, depth, platform_size)
    t.height_field_raw[a:b, a:b] = h


# ---- device descriptors (include/lgsim.h LgTerrainTile): (kind, ip, aux doubles, iaux ints); same draws, same order -------------------
def _d_slope(t, slope=1, platform_size=1.):
    from . import abi
    hs, vs, W = t.horizontal_scale, t.vertical_scale, t.width
    edge = int(0.2 / hs)
    peak = int(slope * (hs / vs) * ((W - 2 * edge) / 2))
    return (abi.TILE_SLOPE, [peak, edge, int(platform_size / hs / 2), 0, 0], [], [])


def _d_uniform(t, min_height, max_height, step=1, downsampled_scale=None):
    """The spline is fitted here and evaluated there."""
    from . import abi
    edge, spline, xs, ys = _uniform_spline(t, min_height, max_height, step, downsampled_scale)
    tx, ty = spline.get_knots()
    aux = np.concatenate([tx, ty, spline.get_coeffs(), xs, ys]).astype(np.float64)
    return (abi.TILE_UNIFORM, [edge, len(tx), len(ty), len(xs), len(ys)], aux, [])


def _d_stairs(t, step_width, step_height, platform_size=1.):
    from . import abi
    _check_stairs(t, step_width)
    hs = t.horizontal_scale
    return (abi.TILE_STAIRS, [int(step_width / hs), int(step_height / t.vertical_scale), int(platform_size / hs), 0, 0], [], [])


def _d_obstacles(t, max_height, min_size, max_size, num_rects, platform_size=1.):
    from . import abi
    rects = _obstacle_rects(t, max_height, min_size, max_size, num_rects)
    return (abi.TILE_OBSTACLES, [len(rects), int(platform_size / t.horizontal_scale), 0, 0, 0], [], [v for r in rects for v in r])


def _d_wave(t, num_waves=1, amplitude=1.):
    """The two float64 factors are numpy's; the kernel adds them (one rounding, as numpy) and truncates to int16."""
    from . import abi
    edge, cy, sx = _wave_rows(t, num_waves, amplitude)
    if cy is None:
        return (abi.TILE_WAVE, [edge, 0, 0, 0, 0], [], [])
    n = t.width - 2 * edge
    assert cy.size == sx.size == n > 0
    return (abi.TILE_WAVE, [edge, n, 0, 0, 0], np.concatenate([cy.ravel(), sx.ravel()]).astype(np.float64), [])


def _d_stones(t, stone_size, stone_distance, max_height, platform_size=1., depth=-10):
    from . import abi
    bg, rects, (a, b) = _stone_rects(t, stone_size, stone_distance, max_height, platform_size, depth)
    rects = [r for r in rects if r[2] > 0 and r[3] > 0]          # the empty "first hole" rectangles only consumed a draw
    return (abi.TILE_STONES, [len(rects), a, b, bg, 0], [], [v for r in rects for v in r])


def _d_gap(t, gap_size, platform_size=1.):
    from . import abi
    (a, b), (c, d) = _gap_spans(t, gap_size, platform_size)
    return (abi.TILE_GAP, [a, b, c, d, 0], [], [])


def _d_pit(t, depth, platform_size=1.):
    from . import abi
    (a, b), h = _pit_span(t, depth, platform_size)
    return (abi.TILE_PIT, [a, b, h, 0, 0], [], [])


# terrain_utils.<name> -> (host generator, device descriptor); the eight heightfield generators selected mode accepts
_GENERATORS = {
    "random_uniform_terrain": (_random_uniform, _d_uniform),
    "pyramid_sloped_terrain": (_pyramid_slope, _d_slope),
    "discrete_obstacles_terrain": (_discrete_obstacles, _d_obstacles),
    "wave_terrain": (_wave, _d_wave),
    "pyramid_stairs_terrain": (_pyramid_stairs, _d_stairs),
    "stepping_stones_terrain": (_stepping_stones, _d_stones),
    "gap_terrain": (_gap, _d_gap),
    "pit_terrain": (_pit, _d_pit),
}


class Terrain:
    def __init__(self, cfg, device=None):
        """device: None = numpy on the host; a HIP device = the tiles are evaluated there (lg_terrain_generate) and `heightsamples_dev`
        holds the int16 grid on that device (`height_field_raw` / `heightsamples` then are its host copy).

        Selected mode (cfg.selected, terrain.py:104-117) calls the generator named by cfg.terrain_kwargs["type"] (matched on the part
        after the last dot, e.g. "terrain_utils.pyramid_stairs_terrain") with the remaining kwargs on every tile.  Unlike the
        reference, which pops "type" out of the config (so a second construction from the same config fails), the user's
        terrain_kwargs are left unchanged."""
        self.cfg, self.type = cfg, cfg.mesh_type
        self._device, self._tiles = device, []
        if self.type in ("none", "plane"):
            return
        if self.type != "heightfield":
            raise NotImplementedError("only heightfield terrain is generated by this backend")
        self.env_length, self.env_width, self.platform_size = cfg.terrain_length, cfg.terrain_width, cfg.platform_size
        self.proportions = [np.sum(cfg.terrain_proportions[:i + 1]) for i in range(len(cfg.terrain_proportions))]
        self.env_origins = np.zeros((cfg.num_rows, cfg.num_cols, 3))
        self.width_per_env_pixels = int(self.env_width / cfg.horizontal_scale)
        self.length_per_env_pixels = int(self.env_length / cfg.horizontal_scale)
        self.border = int(cfg.border_size / cfg.horizontal_scale)
        self.tot_cols = int(cfg.num_cols * self.width_per_env_pixels) + 2 * self.border
        self.tot_rows = int(cfg.num_rows * self.length_per_env_pixels) + 2 * self.border
        self.height_field_raw = np.zeros((self.tot_rows, self.tot_cols), dtype=np.int16)
        self.heightsamples_dev = None
        if cfg.curriculum and cfg.selected:
            raise ValueError("Curriculum and selected terrain cannot be both True.")
        if cfg.curriculum:      # terrain.py:95-102: difficulty along rows (x), type along columns (y)
            for j in range(cfg.num_cols):
                for i in range(cfg.num_rows):
                    self._place(self._make(j / cfg.num_cols + 0.001, i / cfg.num_rows), i, j)
        elif cfg.selected:      # terrain.py:104-117
            name, kwargs = self._selected(cfg.terrain_kwargs)
            for k in range(cfg.num_rows * cfg.num_cols):
                i, j = np.unravel_index(k, (cfg.num_rows, cfg.num_cols))
                self._place(self._tile(name, kwargs), i, j)
        else:                   # terrain.py:85-93
            for k in range(cfg.num_rows * cfg.num_cols):
                i, j = np.unravel_index(k, (cfg.num_rows, cfg.num_cols))
                choice = np.random.uniform(0, 1)
                difficulty = np.random.choice([0.5, 0.75, 0.9])
                self._place(self._make(choice, difficulty), i, j)
        if device is not None:
            self._generate_on_device()
        self.heightsamples = self.height_field_raw

    @staticmethod
    def _selected(terrain_kwargs):
        if not terrain_kwargs or "type" not in terrain_kwargs:
            raise ValueError("selected terrain needs terrain_kwargs with a 'type' entry")
        name = str(terrain_kwargs["type"]).rsplit(".", 1)[-1]
        if name not in _GENERATORS:
            raise NotImplementedError(f"selected terrain type {terrain_kwargs['type']!r}: only the heightfield generators "
                                      f"{sorted(_GENERATORS)} are supported by this backend")
        return name, {k: v for k, v in terrain_kwargs.items() if k != "type"}

    def _make(self, choice, difficulty):
        """terrain.py:119-183: the eight-way dispatch with the reference's parameters.  A choice beyond the last cumulative proportion
        fails on `p[k]` (IndexError) as in the reference; with seven or more entries the last branch is the pit."""
        p, plat = self.proportions, self.platform_size
        slope, step_h, obst_h = difficulty * 0.4, 0.05 + 0.15 * difficulty, 0.05 + difficulty * 0.15
        stone_size, stone_distance = 1.5 * (1.05 - difficulty), 0.05 if difficulty == 0 else 0.1
        gap_size, pit_depth = 1. * difficulty, 0.3 * difficulty
        if choice < p[0]:
            return self._tile("pyramid_sloped_terrain", dict(slope=-slope if choice < p[0] / 2 else slope, platform_size=plat))
        if choice < p[1]:
            return self._tile("random_uniform_terrain", dict(min_height=-0.05, max_height=0.05, step=0.005, downsampled_scale=0.2))
        if choice < p[3]:
            return self._tile("pyramid_stairs_terrain", dict(step_width=0.4, step_height=-step_h if choice < p[2] else step_h, platform_size=plat))
        if choice < p[4]:
            return self._tile("discrete_obstacles_terrain", dict(max_height=obst_h, min_size=1., max_size=2., num_rects=20, platform_size=plat))
        if choice < p[5]:
            return self._tile("stepping_stones_terrain", dict(stone_size=stone_size, stone_distance=stone_distance, max_height=0.,
                                                              platform_size=plat))
        if choice < p[6]:
            return self._tile("gap_terrain", dict(gap_size=gap_size, platform_size=plat))
        return self._tile("pit_terrain", dict(depth=pit_depth, platform_size=plat))

    def _tile(self, name, kwargs):
        """One sub-terrain: its pixels on the host, or its descriptor (the draws taken, the pixels left to the kernel) on the device path."""
        t = _Tile(self.width_per_env_pixels, self.cfg.vertical_scale, self.cfg.horizontal_scale)
        host, describe = _GENERATORS[name]
        if self._device is not None:
            return describe(t, **kwargs)
        host(t, **kwargs)
        return t

    def _generate_on_device(self):
        import ctypes as C
        import torch
        from . import abi
        lib = abi.load_lib()
        need = max(desc[0] for desc, _, _ in self._tiles)
        if need > abi.TILE_OBSTACLES and (not hasattr(lib, "lg_terrain_max_kind") or lib.lg_terrain_max_kind() < need):
            raise RuntimeError(f"{abi.lib_path()} predates terrain tile kind {need} (stepping stones / gap / pit / wave) and would leave "
                               "those tiles flat: rebuild it (`python -c 'import __graft_entry__ as g; g.build()'`)")
        dev = torch.device(self._device)
        tiles = (abi.LgTerrainTile * len(self._tiles))()
        aux, iaux = [], []
        for k, (desc, i, j) in enumerate(self._tiles):
            kind, ip, a, ia = desc
            tiles[k].kind, tiles[k].row, tiles[k].col = kind, i, j
            for q, v in enumerate(ip):
                tiles[k].ip[q] = int(v)
            tiles[k].aux_off = len(iaux) if kind in abi.TILE_IAUX_KINDS else sum(len(x) for x in aux)
            if len(a):
                aux.append(np.asarray(a, np.float64))
            iaux += list(ia)
        raw = np.frombuffer(bytes(tiles), dtype=np.uint8).copy()
        d_tiles = torch.from_numpy(raw).to(dev)
        d_aux = torch.from_numpy(np.concatenate(aux) if aux else np.zeros(1)).to(dev)
        d_iaux = torch.tensor(iaux if iaux else [0], dtype=torch.int32, device=dev)
        hf = torch.empty((self.tot_rows, self.tot_cols), dtype=torch.int16, device=dev)
        oz = torch.empty(len(self._tiles), dtype=torch.float64, device=dev)
        hs = self.cfg.horizontal_scale
        o1, o2 = int((self.env_length / 2. - 1) / hs), int((self.env_length / 2. + 1) / hs)
        assert (o1, o2) == (int((self.env_width / 2. - 1) / hs), int((self.env_width / 2. + 1) / hs)) and self.width_per_env_pixels == self.length_per_env_pixels
        abi.check(lib.lg_terrain_generate(d_tiles.data_ptr(), len(self._tiles), d_aux.data_ptr(), d_iaux.data_ptr(), hf.data_ptr(), self.tot_rows,
                                          self.tot_cols, self.width_per_env_pixels, self.border, o1, o2, float(self.cfg.vertical_scale), oz.data_ptr(),
                                          torch.cuda.current_stream(dev).cuda_stream), lib)
        self.heightsamples_dev = hf
        self.height_field_raw = hf.cpu().numpy()
        z = oz.cpu().numpy()
        for k, (_, i, j) in enumerate(self._tiles):
            self.env_origins[i, j] = [(i + 0.5) * self.env_length, (j + 0.5) * self.env_width, z[k]]

    def _place(self, t, i, j):
        """terrain.py:185-203: paste the tile, origin height = max over the central 2 m x 2 m."""
        if self._device is not None:
            self._tiles.append((t, i, j))      # `t` is the tile's descriptor here; pixels and origin height come from the kernel
            return
        x0 = self.border + i * self.length_per_env_pixels
        y0 = self.border + j * self.width_per_env_pixels
        self.height_field_raw[x0:x0 + self.length_per_env_pixels, y0:y0 + self.width_per_env_pixels] = t.height_field_raw
        hs = t.horizontal_scale
        x1, x2 = int((self.env_length / 2. - 1) / hs), int((self.env_length / 2. + 1) / hs)
        y1, y2 = int((self.env_width / 2. - 1) / hs), int((self.env_width / 2. + 1) / hs)
        z = np.max(t.height_field_raw[x1:x2, y1:y2]) * t.vertical_scale
        self.env_origins[i, j] = [(i + 0.5) * self.env_length, (j + 0.5) * self.env_width, z]
