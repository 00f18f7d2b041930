"""CPU-only tests of the obstacle-map generator's oracle and of the host side of dgp_obstacle_maps.

  * tests/obstacles_oracle.py against the reference's own maps (tests/golden/g11_obstacles.npz, made by tests/golden/make_obstacles_golden.py from the real
    generate_rect_obstacle_map / generate_wall_obstacle_map with every candidate of random_rect / random_wall recorded): fed the recorded candidates, the oracle's
    placement rule gives each map bit for bit and consumes exactly as many candidates -- among them cases whose padded boxes wrap at the low edge;
  * the recorded candidates stay inside the coordinate ranges the oracle draws its own candidates from, and reach both ends of them;
  * the Philox candidates are counter-based and cover the ranges; hand-made cases for the cap, overlap and wrap flags;
  * dataset_params against the numbers of generate_2d_dataset.py:29-75 for im_size 128 and 256;
  * the inputs of the GPU tests (tests/obstacles_cases.py) take every branch and cap nowhere;
  * argument validation of dgp_obstacle_maps (nothing touches a device), the struct layout, the symbol, and the front end's refusal of host tensors."""
import ctypes as C
import os

import numpy as np
import pytest

import obstacles_cases as OC
import obstacles_oracle as OO
from dgpmp2_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fixture_case(g, c):
  kind, side, n = [int(v) for v in g[c + '_params'][:3]]
  p = [int(v) for v in g[c + '_params'][3:]]
  patch, patch_obs = [float(v) for v in g[c + '_patch']]
  gen = OO.Gen(kind, n, n + 1, p[0], p[1], p[2], p[3], p[4], p[5], p[6], p[7], patch, patch_obs, max_draws=1 << 30)      # (the reference has no cap)
  cands = [tuple(int(v) for v in row) for row in g[c + '_cands']]
  return gen, side, n, cands, g.get(c + '_start_pts'), g.get(c + '_goal_pts')


def test_recorded_candidates_give_the_reference_maps_bit_for_bit(golden):
  g = golden('g11_obstacles')
  cases = [str(c) for c in g['cases']]
  assert len(cases) >= 100
  kinds, sides, wrapped, with_pts, rejected = set(), set(), 0, 0, 0
  for c in cases:
    gen, side, n, cands, sp, gp = _fixture_case(g, c)
    taken = []

    def feed(i, it=iter(cands), taken=taken):      # the reference draws every candidate of a map from ONE stream
      for cand in it:
        taken.append(cand)
        yield cand
    m, boxes, draws, info = OO.place(side, side, gen, n, feed, sp, gp)
    want = g[c + '_map']
    assert want.dtype == np.uint8 and np.array_equal(OO.image_of(m, np.uint8), want), c
    assert np.array_equal(OO.image_of(m, np.float64), want.astype(np.float64)), c      # the reference's 1 - count itself
    assert len(taken) == len(cands) and sum(draws) + n == len(cands), (c, len(taken), len(cands))      # exactly as many candidates
    assert not info & 3 and len(boxes) == n * (2 if gen.kind == OO.WALL else 1), c
    kinds.add(gen.kind); sides.add(side)
    wrapped += bool(info & 4) and sp is None      # (without points only a candidate's own box sets the bit)
    with_pts += sp is not None
    rejected += len(cands) - n
  assert kinds == {OO.RECT, OO.WALL} and sides == {32, 64} and with_pts >= 40 and wrapped >= 10 and rejected >= 500


def test_a_wrapped_padded_box_is_an_empty_slice_and_its_check_vacuous(golden):
  """The quirk itself, in the fixture: some accepted rectangle's padded box has a negative bound, NumPy makes an empty slice of it, and the rectangle went in although
  its padded box -- had it been clipped instead -- would have lain on an obstacle placed before."""
  g = golden('g11_obstacles')
  vacuous = 0
  for c in [str(c) for c in g['cases'] if str(c).startswith('wrap') and str(c).endswith('nopts')]:
    gen, side, n, cands, _, _ = _fixture_case(g, c)
    m, boxes, draws, info = OO.place(side, side, gen, n, lambda i, it=iter(cands): it)
    acc, k = [], -1
    for d in draws:
      k += d + 1
      acc.append(cands[k])
    pad = OO.half(gen.patch_size_obs)
    seen = np.zeros((side, side), np.int32)
    for cand in acc:
      (rs, cs), = OO.rect_slices(cand, pad)
      if OO.has_negative_bound([(rs, cs)]) and seen[rs, cs].size == 0:
        clipped = seen[max(rs.start, 0):rs.stop, max(cs.start, 0):cs.stop]
        vacuous += bool(clipped.any())
      OO.paint(seen, OO.rect_slices(cand))
  assert vacuous >= 1


def test_recorded_candidates_stay_in_the_ranges_and_reach_both_ends(golden):
  g = golden('g11_obstacles')
  ends = {}
  for c in [str(c) for c in g['cases']]:
    gen, side, n, cands, _, _ = _fixture_case(g, c)
    x_hi, y_hi = (side, side) if gen.kind == OO.WALL else (gen.end_x, gen.end_y)
    e = ends.setdefault(gen.kind, set())
    for w, h, cx, cy in cands:
      ranges = ((w, gen.w_min, gen.w_max), (h, gen.h_min, gen.h_max), (cx, gen.start_x + OO.half(w), x_hi - OO.half(w)), (cy, gen.start_y + OO.half(h), y_hi - OO.half(h)))
      for f, (v, lo, hi) in enumerate(ranges):
        assert lo <= v <= hi, (c, f, v, lo, hi)
        if v == lo: e.add((f, 'lo'))
        if v == hi: e.add((f, 'hi'))
  for kind in (OO.RECT, OO.WALL):
    assert ends[kind] == {(f, s) for f in range(4) for s in ('lo', 'hi')}, (kind, sorted(ends[kind]))


def test_philox_candidates_are_counter_based_and_cover_the_ranges():
  for gen, H, W in ((OC.gens_of('multi_obs', 32)[0], 32, 37), (OC.gens_of('passage', 32)[0], 32, 37)):
    x_hi, y_hi = (W, H) if gen.kind == OO.WALL else (gen.end_x, gen.end_y)
    cands = [OO.candidate(gen, H, W, 3, 5, i, k) for i in range(4) for k in range(600)]
    assert len(set(cands)) > 1000
    seen = set()
    for w, h, cx, cy in cands:
      for f, (v, lo, hi) in enumerate(((w, gen.w_min, gen.w_max), (h, gen.h_min, gen.h_max), (cx, gen.start_x + OO.half(w), x_hi - OO.half(w)),
                                       (cy, gen.start_y + OO.half(h), y_hi - OO.half(h)))):
        assert lo <= v <= hi
        if v in (lo, hi): seen.add((f, v == lo))
    assert len(seen) == 8
    a = OO.candidate(gen, H, W, 3, 5, 1, 9)
    assert a == OO.candidate(gen, H, W, 3, 5, 1, 9)
    assert len({a, OO.candidate(gen, H, W, 4, 5, 1, 9), OO.candidate(gen, H, W, 3, 6, 1, 9), OO.candidate(gen, H, W, 3, 5, 2, 9), OO.candidate(gen, H, W, 3, 5, 1, 10),
                OO.candidate(gen, H, W, 3, (1 << 40) + 5, 1, 9), OO.candidate(gen, H, W, 3 + (1 << 35), 5, 1, 9)}) == 7      # seed and environment: both words of each
  # the count comes from the half-open range, the generator of a mixed type from all of them
  gens = OC.gens_of('mixed', 32)
  picks = [OO.count_and_generator(gens, 9, e) for e in range(300)]
  assert {p[1] for p in picks} == set(gens)
  for gen in gens:
    assert {p[0] for p in picks if p[1] is gen} == set(range(gen.n_lo, gen.n_hi))
  assert OO.draw_in(0, 3, 9) == 3 and OO.draw_in(0xffffffff, 3, 9) == 9 and OO.draw_in(1 << 31, 0, 1) == 1 and OO.draw_in((1 << 31) - 1, 0, 1) == 0


def test_the_flags_on_hand_made_cases():
  rect = lambda **kw: OO.Gen('rect', 1, 2, 2, 4, 2, 4, 0, 0, 15, 15, **kw)
  feed = lambda *cands: (lambda i, it=iter(cands): it)
  # cap: nothing but the spot that is taken -- after max_draws candidates the last one goes in, on top
  m, boxes, draws, info = OO.place(16, 16, rect(max_draws=3), 2, feed((4, 4, 8, 8), (4, 4, 8, 8), (4, 4, 9, 9), (2, 2, 8, 7)))
  assert draws == [0, 2] and info == 1 | 2 and boxes == [[6, 10, 6, 10], [6, 8, 7, 9]] and m.max() == 2
  # ... and a free spot as the last candidate is simply accepted
  m, boxes, draws, info = OO.place(16, 16, rect(max_draws=3), 2, feed((4, 4, 8, 8), (4, 4, 8, 8), (4, 4, 9, 9), (2, 2, 2, 2)))
  assert draws == [0, 2] and info == 0 and m.max() == 1
  # wrap: the padded box of a rectangle at the low edge is rows [-2, 4): NumPy reads [14, 4), empty -- the check is vacuous, the twin goes in on top (overlap, no cap)
  m, boxes, draws, info = OO.place(16, 16, rect(patch_size_obs=4.0, max_draws=3), 2, feed((2, 2, 1, 1), (2, 2, 1, 1)))
  assert draws == [0, 0] and info == 2 | 4 and boxes == [[0, 2, 0, 2], [0, 2, 0, 2]] and m[0, 0] == 2
  # ... after which nothing is valid any more, wherever it lies
  m, boxes, draws, info = OO.place(16, 16, rect(patch_size_obs=4.0, max_draws=2), 3, feed((2, 2, 1, 1), (2, 2, 1, 1), (2, 2, 10, 10), (2, 2, 12, 5)))
  assert draws == [0, 0, 1] and info == 1 | 2 | 4 and boxes[2] == [4, 6, 11, 13]
  # clamping without a wrap: the padded box over the HIGH edge is clipped and still keeps its distance
  m, boxes, draws, info = OO.place(16, 16, rect(patch_size_obs=4.0, max_draws=8), 2, feed((2, 2, 14, 14), (2, 2, 13, 11), (2, 2, 14, 10)))
  assert draws == [0, 1] and info == 0
  # a keep-out patch: rows and columns [ceil(v) - 2, ceil(v) + 2); one at the low edge wraps (bit 2 without any obstacle)
  pts = np.array([[7.3, 8.0]])
  m, boxes, draws, info = OO.place(16, 16, rect(patch_size=4.0, max_draws=8), 1, feed((2, 2, 9, 9), (2, 2, 11, 9)), pts, None)
  assert draws == [1] and info == 0      # columns [6, 10) of the patch meet [8, 10) of the first candidate, not [10, 12) of the second
  assert OO.place(16, 16, rect(patch_size=4.0), 0, feed(), None, np.array([[0.5, 9.0]]))[3] == 4
  # a wall is two boxes; its gap stays open
  wall = OO.Gen('wall', 1, 2, 2, 4, 2, 4, 1, 0, max_draws=4)
  m, boxes, draws, info = OO.place(16, 12, wall, 1, feed((4, 3, 6, 8)))
  assert boxes == [[0, 6, 4, 8], [10, 16, 4, 8]] and info == 0 and m[:, 4:8].sum(1).tolist() == [4] * 6 + [0] * 4 + [4] * 6


def test_dataset_params_equal_the_reference_numbers():
  """generate_2d_dataset.py:29-75 evaluated by hand for im_size 128 and 256"""
  from dgpmp2_amd.datasets.obstacle_maps import dataset_params, reference_separations
  want = {
      ('tar_pit', 128): ('rect', 5, 8, 12, 13, 12, 13, 19, 19, 83, 83), ('tar_pit', 256): ('rect', 5, 8, 25, 26, 25, 26, 38, 38, 166, 166),
      ('forest', 128): ('rect', 23, 45, 4, 5, 4, 5, 0, 0, 127, 127), ('forest', 256): ('rect', 23, 45, 8, 9, 8, 9, 0, 0, 255, 255),
      ('multi_obs', 128): ('rect', 2, 5, 16, 26, 16, 26, 12, 12, 115, 115), ('multi_obs', 256): ('rect', 2, 5, 32, 42, 32, 42, 25, 25, 230, 230),
      ('passage', 128): ('wall', 1, 2, 25, 35, 9, 10, 19, 0, 0, 0), ('passage', 256): ('wall', 1, 2, 51, 61, 9, 10, 38, 0, 0, 0)}
  keys = ('kind', 'n_lo', 'n_hi', 'w_min', 'w_max', 'h_min', 'h_max', 'start_x', 'start_y', 'end_x', 'end_y')
  for (t, size), w in want.items():
    p = dataset_params(t, size, 7.0, 9.5)      # (the passage size 9.5 is truncated: int(passage_size))
    assert tuple(p[k] for k in keys) == w, (t, size)
    assert p['patch_size'] == 7.0 and p['patch_size_obs'] == (0.0 if t == 'passage' else 9.5)
  mixed = dataset_params('mixed_clutter', 128, 7.0, 9.5)
  assert [tuple(p[k] for k in keys) for p in mixed] == [want[(t, 128)] for t in ('tar_pit', 'forest', 'multi_obs')]
  with pytest.raises(ValueError):
    dataset_params('maze', 128, 1.0, 1.0)
  # :151-154, :196-208 with the example configuration: radius 0.4, epsilon 0.4, 10 m over 128 cells -> patch_size_robot 6, patch_size_safety 11
  assert reference_separations('tar_pit', 0.4, 0.4, (-5.0, 5.0), 128) == (28.0, 0.0) and reference_separations('forest', 0.4, 0.4, (-5.0, 5.0), 128) == (18.0, 18)
  assert reference_separations('multi_obs', 0.4, 0.4, (-5.0, 5.0), 128) == (17, 34.0) and reference_separations('passage', 0.4, 0.4, (-5.0, 5.0), 128) == (18.0, 24.0)


def test_confs_to_pixels():
  import torch
  from dgpmp2_amd.datasets.obstacle_maps import confs_to_pixels
  confs = torch.tensor([[[-5.0, 5.0, 0.0, 0.0], [0.0, 0.0, 1.0, 1.0], [2.5, -1.25, 0.0, 0.0]]], dtype=torch.float64)
  px = confs_to_pixels(confs, (-5.0, 5.0), (-5.0, 5.0), 128)
  assert px.dtype == torch.float64 and px.shape == (1, 3, 2) and px.tolist() == [[[0.0, 0.0], [64.0, 64.0], [96.0, 80.0]]]      # x from the left, y from the top


@pytest.mark.parametrize('name', sorted(OC.CASES))
def test_gpu_test_inputs_cap_nowhere(name):
  count, boxes, num_boxes, draws, info = OC.expected(name)
  assert not (info & 1).any(), 'the oracle caps environments %s' % np.flatnonzero(info & 1)


def test_gpu_test_inputs_take_every_branch():
  ex = {name: OC.expected(name) for name in OC.CASES}
  kinds = {name: OC.gens_of(OC.CASES[name][0], 32)[0].kind for name in OC.CASES}
  assert OO.WALL in kinds.values() and OO.RECT in kinds.values()
  assert any(OC.CASES[n][4] > 0 and kinds[n] == OO.WALL for n in OC.CASES) and any(OC.CASES[n][4] > 0 and kinds[n] == OO.RECT for n in OC.CASES)
  assert any(OC.CASES[n][4] == 0 for n in OC.CASES)
  assert (ex['small_forest44_high_env'][2] == 44).all() and max(e[2].max() for n, e in ex.items() if n.startswith('main')) == 44      # 44 obstacles
  assert OC.CASES['small_forest44_high_env'][3] > 1 << 32
  for n in ('small_wrap', 'small_wrap_no_points'):      # a wrapped box was accepted; without points nothing else sets the bit
    assert (ex[n][4] & 4).any()
  assert (ex['small_wrap_no_points'][4] & 2).any() and not (ex['small_wrap_no_points'][4] & 4).all()      # an overlap behind a vacuous check (on the last obstacle: no cap)
  assert max(e[3].max() for e in ex.values()) >= 64      # an accepted draw beyond the first round of 64 candidates
  assert any((e[3][:, 0] > 0).any() for e in ex.values()) and any((e[3][:, 0] == 0).any() for e in ex.values())
  mixed = ex['main_mixed'][2]
  assert (mixed <= 7).any() and (mixed >= 23).any()      # several generators in one batch
  for n, e in ex.items():      # walls: two boxes each
    if kinds[n] == OO.WALL: assert (e[2] == 2 * (e[3] >= 0).sum(1)).all()


# ---- the entry point, without a GPU -------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def api():
  if not os.path.exists(_capi.LIB_PATH):
    import __graft_entry__
    __graft_entry__.build()
  return _capi.get_api()


def _solver():
  return _capi.Solver(_capi.make_config(num_states=16, dof=2, io_dtype=_capi.DGP_F64, total_time_sec=10.0, x_lims=(-5, 5), y_lims=(-5, 5), K_s=0.01, K_g=0.01, reg=0.1,
                                        sphere_radius=0.4, Q_c_inv=[[1, 0], [0, 1]], cost_sigma=0.01, epsilon_dist=0.4))


def test_struct_layout_symbol_and_header(api):
  P = _capi.DgpObstacleParams
  assert C.sizeof(P) == 12 * 4 + 2 * 8      # include/dgpmp2_hip.h: twelve int32, two doubles
  assert [f[0] for f in P._fields_] == ['kind', 'n_lo', 'n_hi', 'w_min', 'w_max', 'h_min', 'h_max', 'start_x', 'start_y', 'end_x', 'end_y', 'max_draws', 'patch_size_obs',
                                        'patch_size']
  assert P.max_draws.offset == 44 and P.patch_size_obs.offset == 48 and P.patch_size.offset == 56
  assert 'obstacle_maps' in _capi.CApi.SYMBOLS and api.obstacle_maps is not None and api.abi_version() == 7
  header = open(os.path.join(ROOT, 'include', 'dgpmp2_hip.h')).read()
  assert 'int dgp_obstacle_maps(const DgpHandle* h' in header and 'typedef struct DgpObstacleParams' in header and 'obst_generator.py:179-221' in header
  assert '#define DGP_OBST_MAX_BOXES      64' in header and (_capi.DGP_OBST_MAX_BOXES, _capi.DGP_OBST_MAX_POINTS) == (OO.MAX_BOXES, OO.MAX_POINTS) == (64, 32)
  from dgpmp2_amd._build.units import UNITS
  assert any(u.name == 'obstacle_maps' and u.source == 'obstacle_maps.hip' and u.launcher is None for u in UNITS)


def test_obstacle_maps_validates_arguments_without_gpu(api):
  s = _solver()
  ok = dict(kind=_capi.DGP_OBST_RECT, n_lo=5, n_hi=8, w_min=3, w_max=4, h_min=3, h_max=4, start_x=4, start_y=4, end_x=20, end_y=20, patch_size_obs=0.0, patch_size=4.0)
  wall = dict(kind=_capi.DGP_OBST_WALL, n_lo=1, n_hi=2, w_min=6, w_max=16, h_min=4, h_max=5, start_x=4, start_y=0, patch_size=3.0)
  mk = lambda base=ok, **kw: s.obstacle_params(**dict(base, **kw))

  def refused(params, batch=8, rows=32, cols=32, image=0x1000, **kw):
    with pytest.raises(_capi.DgpError) as e:
      s.obstacle_maps(batch, rows, cols, params, image, **kw)
    assert e.value.code == _capi.DGP_EINVAL
    return str(e.value)
  refused(None)                                                          # NULL params
  refused(mk(), image=None)                                              # NULL output
  assert 'boxes' in refused(mk(n_hi=66))                                 # 65 rectangles
  assert 'boxes' in refused(mk(wall, n_hi=34))                           # 33 walls are 66 boxes
  assert 'empty' in refused(mk(n_lo=5, n_hi=5)) and 'empty' in refused(mk(n_lo=-1))
  assert 'keep-out' in refused(mk(), start_pts=0x1000, goal_pts=0x1000, num_pts=33)
  assert 'max_draws' in refused(mk(max_draws=0))
  assert 'coordinate range' in refused(mk(start_x=10, end_x=13))        # cx in [10 + 2, 13 - 2] for a width of 3 or 4: randint raises in the reference
  assert 'coordinate range' in refused(mk(start_y=19))
  assert 'coordinate range' in refused(mk(wall), cols=19)               # a wall of width 16 in [4 + 8, 19 - 8]
  assert 'coordinate range' in refused(mk(wall, start_y=28))            # gap_y + ceil(5 / 2) beyond rows - ceil(5 / 2)
  assert 'size ranges' in refused(mk(w_min=5)) and 'size ranges' in refused(mk(h_min=-1))
  assert 'NaN' in refused(mk(patch_size_obs=float('nan'))) and 'NaN' in refused(mk(patch_size=float('nan')))
  assert 'kind' in refused(mk(kind=2))
  assert 'image_dtype' in refused(mk(), image_dtype=3)
  assert 'aligned' in refused(mk(), image=0x1004, image_dtype=_capi.DGP_F64)
  refused(mk(), batch=0); refused(mk(), rows=0); refused(mk(), cols=-3)
  refused([mk()] * 5); refused([])                                       # 1 .. 4 generators
  assert 'coordinate range' in refused([mk(), mk(start_x=10, end_x=13)])  # every generator is checked
  p = mk()
  assert api.obstacle_maps(None, 8, 32, 32, C.byref(p), 1, 0, 0, None, None, 0, 0x1000, _capi.DGP_U8, None, None, None, None, None) == _capi.DGP_EINVAL      # handle
  assert b'null handle' in api.last_error()


def test_front_end_refuses_host_tensors():
  import torch
  from dgpmp2_amd import datasets as D
  assert D.generate_obstacle_maps is not None and D.ObstacleInfo is not None and D.dataset_params is not None and D.confs_to_pixels is not None
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    D.generate_obstacle_maps(object(), 'forest', 2, 32, start_pts=torch.zeros(2, 1, 2))
  with pytest.raises(RuntimeError, match='CUDA/ROCm'):
    D.generate_obstacle_maps(object(), 'forest', 2, 32, goal_pts=np.zeros((2, 1, 2)))
  with pytest.raises(TypeError):
    D.generate_obstacle_maps(object(), 'forest', 2, 32, dtype=torch.int32)
  with pytest.raises(ValueError, match='dataset_type'):
    D.generate_dataset('unused', 'train', None, None, 1)
  flags = torch.tensor([0, 1, 2, 4, 7], dtype=torch.int32)
  info = D.ObstacleInfo(None, None, None, flags)
  assert info.capped.tolist() == [False, True, False, False, True] and info.overlapping.tolist() == [False, False, True, False, True]
  assert info.wrapped.tolist() == [False, False, False, True, True]
