"""The scratch-memory contract of the C ABI (include/rigl_hip.h: "scratch comes from a caller-provided workspace
(`*_workspace_bytes`)") for everything outside the K1 exact walk, which has its own --workspace exact (tests/k1_exact.py):
batch norm, the fused stem tail, K2 and the K-split forward.

Every case runs through ``rigl_amd.ops`` with ``ops.workspace`` replaced by tests/wsguard.py: each request exactly as long as
the size query said, between two 1 MiB guards, pre-filled with 0x00 and then with 0xFF.  Per poison the case is held to the
reference that already pins it, under that reference's own criterion (the helpers of tests/test_bn_edges_gpu.py and
tests/bn_ref.py, tests/glue_ref.py, tests/test_k2_prune_regrow_gpu.py and oracle.rigl_oracle are imported, not restated);
after the run every guard must be intact; and the outputs of the two poison runs must agree BIT FOR BIT.

Kernels exempt from the bit-for-bit agreement (an order-dependent floating-point accumulation in their source): none.
Every atomic in rigl_amd/csrc adds integers (prune_regrow.hip:245-253, 365, 548, 777-778, 905, 1171: histogram bins and
counters; head.hip:247-249: hit counts), and every floating-point reduction that goes through a workspace sums its partial
rows in a fixed order (bn.hip k_fwd_finalize / k_bwd_finalize, conv.hip launch_wgrad_reduce, depthwise.hip k_wgrad_final*).

The second half is the error contract, host side only: for every entry point that takes (workspace, workspace_bytes), whose
query is positive at a small shape and whose size check precedes its first launch IN THE SOURCE (the line is named next to
each case), workspace_bytes = need - 1 and workspace = NULL must return RIGL_EWORKSPACE and leave every output at its
sentinel.  No short-workspace call is made whose rejection was not read off the code first.
"""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import rigl_oracle as O  # noqa: E402
from tests import bn_ref as R  # noqa: E402
from tests import exactref as E  # noqa: E402
from tests import glue_ref as GR  # noqa: E402
from tests import k1_check  # noqa: E402
from tests import prune_ref  # noqa: E402
from tests import test_bn_edges_gpu as TB  # noqa: E402
from tests import test_bn_gpu as TBN  # noqa: E402
from tests import test_k2_prune_regrow_gpu as TK  # noqa: E402
from tests import wsguard as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GRID = (4, 32, 32, 64, 128, 1, 2, 0, 0, 16, 16)              # strided 1x1, 1 024 output rows: rigl_masked_conv2d_bwd_grid
_GUARD = []


def _guard():
  if not _GUARD:
    _GUARD.append(G.GuardedWorkspace())
  return _GUARD[0]


def _raw(t):
  if isinstance(t, np.ndarray):
    t = torch.from_numpy(np.ascontiguousarray(t))
  return t.detach().contiguous().reshape(-1).view(torch.uint8).cpu()


def _both_poisons(name, body, want_bytes=None, requests=True):
  """``body()`` -> the case's outputs (tensors / arrays), run once per poison under the guard after holding them to its
  reference itself.  Guards intact after each run; the two runs' outputs bit-identical; ``want_bytes`` (a callable, asked
  under the same knobs): every request is exactly that long.  Returns the [(tag, declared bytes, high-water bytes)] of the
  0xFF run (printed: profiles/workspace/README.md is made of these lines)."""
  g = _guard()
  outs, logs = [], []
  for p in G.POISONS:
    g.poison = p
    with G.installed(g):
      out = body()
      logs.append(g.check('%s [poison 0x%02X]' % (name, p)))
    outs.append([_raw(t) for t in out if t is not None])
  assert [l[:2] for l in logs[0]] == [l[:2] for l in logs[1]], name + ': the two poison runs asked for different workspaces'
  if requests:
    assert logs[0], name + ': no workspace was requested'
  if want_bytes is not None:
    for tag, nbytes, _ in logs[1]:
      assert nbytes == want_bytes, '%s: asked for %d bytes, the query says %d' % (name, nbytes, want_bytes)
  assert len(outs[0]) == len(outs[1])
  for i, (a, b) in enumerate(zip(*outs)):
    assert torch.equal(a, b), '%s: output %d depends on what the workspace held before (0x00 vs 0xFF)' % (name, i)
  print('workspace %s: %s' % (name, [list(l) for l in logs[1]]))
  return logs[1]


# ---------------------------------------------------------------------------------------------------------------------
# batch norm
# ---------------------------------------------------------------------------------------------------------------------
# (rows, channels, parts make_geom gives, is the last part ragged): 1 part, a ragged last part, the 512-part cap, per channel
# count -- c = 8 / 64 / 2048 are 256 / 32 / 1 row lanes per workgroup (bn_ref.geometry restates make_geom)
BN_CASES = [
    (300, 8, 1), (6149, 8, 4), (512 * 2304 - 5, 8, 512),
    (200, 64, 1), (1000, 64, 4), (512 * 288 - 5, 64, 512),
    (8, 2048, 1), (27, 2048, 4), (512 * 9 - 1, 2048, 512),
]


def _bn_bytes(m, c):
  from rigl_amd import _lib
  return int(_lib.load().rigl_bn_workspace_bytes(m, c))


@pytest.mark.parametrize('m,c,parts', BN_CASES, ids=['%dx%d' % t[:2] for t in BN_CASES])
def test_bn_fwd_and_bwd(m, c, parts):
  """bn_fwd (+ residual + ReLU bits) and bn_bwd (+ dres) on bn_ref.edge_tensor.  First the workspace facts, from plain
  calls: the query is the documented layout, every request is exactly the query, guards intact, both poison runs
  bit-identical.  Then test_bn_edges_gpu's checks (its _forward / _backward, unchanged) under the guard, per poison.

  What these shapes found (not a workspace matter): with statistics formed as E[x^2] - mean^2 from fp32 sums of x and
  x^2, 6149x8 and 1179643x8 missed bn_ref's bounds on the variance (measured on an MI355X: moving variance 1.40 of its bound
  and saved invstd 0.77 at 6149x8, saved invstd 1.04 at 1179643x8) on edge_tensor's channel 32 standard deviations from
  zero -- the loss bn_ref.edge_tensor's docstring describes, 2^-24 (mean / std)^2 of the variance per rounding, which the
  suite's other tensors average away over hundreds of short parts; at c = 8 a part is 256 row lanes and 1 792 rows or more,
  and 6149x8 has four of them.  k_reduce now sums x - k and (x - k)^2 around a per-channel pivot k (bn.hip: pivot3), and
  both cases hold the same bounds."""
  from rigl_amd import ops
  rpb, got_parts, rpp = R.geometry(m, c)
  assert got_parts == parts and (parts == 1 or m % rpp), 'the case is not the geometry it is here for'
  need = _bn_bytes(m, c)
  assert need == -(-parts * 2 * c * 4 // 256) * 256 + -(-3 * c * 4 // 256) * 256
  x, dy, res, gamma, beta = TB._inputs((1, 1, m, c))
  name = 'bn %dx%d' % (m, c)

  def body():
    rm, rv = (t.to(DEV) for t in R.moving_start(c, 1))
    y, saved, bits = ops.bn_fwd(x, gamma, beta, rm, rv, 0.1, 1e-5, True, res, want_relu_bits=True)
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx, dres = ops.bn_bwd(x, None, dy, gamma, saved, True, dg, db, want_dres=True, relu_bits=bits)
    y2, saved2 = ops.bn_fwd(x, gamma, beta, None, None, 0.1, 1e-5, False)
    dg2, db2 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx2, _ = ops.bn_bwd(x, None, dy, gamma, saved2, False, dg2, db2)
    return y, saved, bits, rm, rv, dx, dres, dg, db, y2, saved2, dx2, dg2, db2
  _both_poisons(name, body, want_bytes=need)
  st = R.stats_ref(x, 1e-5)
  g = _guard()
  for p in G.POISONS:
    g.poison = p
    with G.installed(g):
      try:
        worst = {}
        y, saved, bits, _ = TB._forward(name, x, res, gamma, beta, 1e-5, 0.1, True, worst, st=st)
        TB._backward(name, x, dy, y, bits, gamma, saved, st, True, True, worst)
        y, saved, _, _ = TB._forward(name, x, None, gamma, beta, 1e-5, 0.1, False, worst, st=st)
        TB._backward(name, x, dy, y, None, gamma, saved, st, False, False, worst)
      finally:
        g.check('%s under the reference checks [poison 0x%02X]' % (name, p))
    TB._show('%s poison 0x%02X' % (name, p), worst)


@pytest.mark.parametrize('parts', [256, 257, 1024, 1025])
def test_bn_fwd_from_producer_partials(parts):
  """The three finalize kernels (bn.hip:664-672: <= 256 parts, <= 1024, above) fed a producer's partial sums.  With
  partials the forward takes NO workspace (include/rigl_hip.h: "with stats the workspace may be NULL"): the wrapper passes
  NULL / 0, so no request is made -- the case pins that this form runs without scratch, under the same checks."""
  c, rows = 64, 4
  m = parts * rows
  x, _, res, gamma, beta = TB._inputs((1, 1, m, c))
  xd = x.double().reshape(parts, rows, c)
  partials = torch.stack([xd.sum(1), (xd * xd).sum(1)], dim=1).float().contiguous()
  name = 'bn_fwd from %d partials' % parts

  def body():
    y, saved, bits, _ = TB._forward(name, x, res, gamma, beta, 1e-5, 0.1, True, {}, partials=partials)
    return y, saved, bits
  assert _both_poisons(name, body, requests=False) == []


@pytest.mark.parametrize('m,c', [(1000, 64), (512 * 9 - 1, 2048)], ids=['1000x64', '4607x2048'])
def test_bn_bwd_reduce_and_statistics(m, c):
  """bn_bwd_reduce (reduce + finalize, the coefficients in the caller's tensor) against bn_bwd's own bits and the float64
  sums behind check_backward; bn_fwd_statistics under check_statistics."""
  from rigl_amd import ops
  x, dy, _, gamma, beta = TB._inputs((1, 1, m, c))
  st = R.stats_ref(x, 1e-5)
  y, saved, bits = ops.bn_fwd(x, gamma, beta, None, None, 0.1, 1e-5, True, None, want_relu_bits=True)
  on = R.unpack_bits(bits, x.shape)
  name = 'bn_bwd_reduce %dx%d' % (m, c)

  def body():
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx, _ = ops.bn_bwd(x, None, dy, gamma, saved, True, dg, db, relu_bits=bits)
    R.check_backward(name, x, dy, on, gamma, st, dx, dg, db)
    dg1, db1 = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    coef = ops.bn_bwd_reduce(x, dy, gamma, saved, True, bits, dg1, db1)
    assert torch.equal(dg, dg1) and torch.equal(db, db1), name + ': not the bits of bn_bwd (same geometry, same order)'
    # a = gamma * invstd (one fp32 product); b = mean dz, c = mean dz * xhat: fp32(s / m) of the float64 sums whose fp32
    # roundings are dbeta / dgamma -- two roundings of 2^-24 apart at most, held to 2^-22
    assert torch.equal(coef[0], gamma * saved[1]), name + ': coef a'
    for row, tot in ((1, db1), (2, dg1)):
      want = tot.double() / m
      assert bool(((coef[row].double() - want).abs() <= 2.0 ** -22 * want.abs() + 1e-44).all()), name + ': coef row %d' % row
    rm0, rv0 = (t.to(DEV) for t in R.moving_start(c, 1))
    rm, rv = rm0.clone(), rv0.clone()
    s2 = ops.bn_statistics(x, gamma, beta, rm, rv, 0.1, 1e-5)
    R.check_statistics(name, st, gamma, beta, s2, rm0, rv0, rm, rv, 0.1)
    assert torch.equal(s2, saved), name + ': bn_statistics is not the statistics half of bn_fwd'
    return dx, dg, db, coef, s2, rm, rv
  _both_poisons(name, body, want_bytes=_bn_bytes(m, c))


@pytest.mark.parametrize('shape', [(33, 3, 3, 40), (1, 1, 1000, 64), (1, 1, 27, 2048)], ids=TB._ids)
def test_bn_add_bn_fwd_and_bwd(shape):
  """The two-batch-norm pair under test_bn_gpu's criterion (bit-identical to the separate calls, which bn_ref pins), on
  edge data; its backward's workspace is two halves (rigl_bn_add_bn_bwd_workspace_bytes)."""
  from rigl_amd import _lib, ops
  m, c = shape[0] * shape[1] * shape[2], shape[3]
  x, dy, _, gamma, beta = (t.to(DEV) for t in R.edge_tensor(m, c, 11))
  x2, _, _, gamma2, beta2 = (t.to(DEV) for t in R.edge_tensor(m, c, 12))
  x2, gamma2 = x2.roll(3, dims=1).contiguous(), gamma2.roll(1)
  assert int(_lib.load().rigl_bn_add_bn_bwd_workspace_bytes(m, c)) == 2 * _bn_bytes(m, c)
  name = 'bn_add_bn %s' % TB._ids(shape)

  def body():
    TBN._pair_equals_separate_calls(x, x2, dy, gamma, gamma2, beta, beta2)
    mk = lambda: (torch.zeros(c, device=DEV), torch.ones(c, device=DEV))   # noqa: E731
    t2 = ops.bn_statistics(x2, gamma2, beta2, *mk(), 0.1, 1e-5)
    y, t1, bits = ops.bn_add_bn_fwd(x, x2, t2, gamma, beta, *mk(), 0.1, 1e-5, True)
    h = [torch.empty(c, device=DEV) for _ in range(4)]
    dx, dx2 = ops.bn_add_bn_bwd(x, x2, bits, dy, gamma, t1, gamma2, t2, *h)
    return [y, t1, t2, bits, dx, dx2] + h
  log = _both_poisons(name, body)
  assert {n for _, n, _ in log} == {_bn_bytes(m, c), 2 * _bn_bytes(m, c)}


def test_bn_query_follows_the_bn_max_parts_knob():
  """"bn_max_parts" raised through ops.tune_set: 1 025 partial rows instead of at most 512 -- the query must follow the knob (the
  kernels write every part they are launched for), and the forward then finalizes through k_fwd_finalize<1>, the backward
  through k_bwd_finalize<4>."""
  from rigl_amd import ops
  m, c = 8 * 1025, 2048
  x, dy, res, gamma, beta = TB._inputs((1, 1, m, c))
  st = R.stats_ref(x, 1e-5)
  default = _bn_bytes(m, c)
  # (at the default cap the 8 200 rows fall into 483 parts of 17; with the cap out of the way, into 1 025 of 8)
  assert R.geometry(m, c)[1] == 483 and R.geometry(m, c, 2048)[1] == 1025
  name = 'bn %dx%d bn_max_parts=2048' % (m, c)
  ops.tune_set('bn_max_parts', 2048)
  try:
    need = _bn_bytes(m, c)
    assert need == 1025 * 2 * c * 4 + 3 * c * 4 and need > default

    def body():
      y, saved, bits, _ = TB._forward(name, x, res, gamma, beta, 1e-5, 0.1, True, {}, st=st)
      dx, dg, db = TB._backward(name, x, dy, y, bits, gamma, saved, st, True, True, {})
      return y, saved, bits, dx, dg, db
    _both_poisons(name, body, want_bytes=need)
  finally:
    ops.tune_unset('bn_max_parts')
  assert _bn_bytes(m, c) == default


# ---------------------------------------------------------------------------------------------------------------------
# the fused stem tail
# ---------------------------------------------------------------------------------------------------------------------
POOL_GEOMS = GR.small_pool_geometries()[:2]                 # the two smallest shapes of tests/test_glue_edges_gpu.py


@pytest.mark.parametrize('gname,d', POOL_GEOMS, ids=[g[0] for g in POOL_GEOMS])
def test_bn_relu_maxpool_fwd_and_bwd(gname, d):
  """ops.bn_relu_maxpool_fwd against glue_ref (maxpool_ref of bn_relu_ref fed the saved scale / shift, as
  test_fused_stem_tail_through_its_wrapper) with its statistics under bn_ref.check_statistics, and _bwd under the criterion
  of test_bn_gpu.test_bn_relu_maxpool_in_one_piece (the three-kernel form), which runs here under the guard as it stands."""
  from rigl_amd import _lib, ops
  from tests import test_glue_edges_gpu as TG
  gd = TG._gdesc(d)
  xc = GR.pool_input('normal', d, 11)
  x, dyp = xc.to(DEV), GR.pool_dy(d, 11).to(DEV)
  c = d.cin
  g = torch.Generator().manual_seed(11)
  gamma = (torch.rand(c, generator=g) + 0.5).to(DEV)
  beta = (torch.randn(c, generator=g) - 1.0).to(DEV)
  st = R.stats_ref(x.reshape(-1, c), 1e-5)
  need = int(_lib.load().rigl_bn_relu_maxpool_bwd_workspace_bytes(C.byref(gd)))
  name = 'bn_relu_maxpool ' + gname

  def body():
    TBN.test_bn_relu_maxpool_in_one_piece((d.n, d.h, d.w, c))
    rm0, rv0 = (t.to(DEV) for t in R.moving_start(c, 1))
    rm, rv = rm0.clone(), rv0.clone()
    y, arg, saved = ops.bn_relu_maxpool_fwd(gd, x, gamma, beta, rm, rv, 0.1, 1e-5)
    R.check_statistics(name, st, gamma, beta, saved, rm0, rv0, rm, rv, 0.1)
    yr, ar = GR.maxpool_ref(GR.bn_relu_ref(xc, saved[2].cpu(), saved[3].cpu()), d)
    assert torch.equal(TG._bits(y), TG._bits(yr)) and torch.equal(arg.cpu(), ar), name + ': y / argmax'
    dg, db = torch.empty(c, device=DEV), torch.empty(c, device=DEV)
    dx = ops.bn_relu_maxpool_bwd(gd, x, dyp, arg, gamma, saved, dg, db)
    return y, arg, saved, rm, rv, dx, dg, db
  log = _both_poisons(name, body)
  assert need in {n for _, n, _ in log}


# ---------------------------------------------------------------------------------------------------------------------
# K2
# ---------------------------------------------------------------------------------------------------------------------
K2_SIZES = (1, 33, 4095, 4096, 4097, 70001)                 # around the 4 096-element chunk; 70 001 = 18 chunks


def _k2_data(n, seed):
  """test_k2_prune_regrow_gpu's heavy-tie data: weights and gradients from a handful of values, so both thresholds cut
  through long runs of equals and the tie-count regions of the workspace carry data."""
  rs = np.random.RandomState(seed)
  mask = (rs.rand(n) < 0.3).astype(np.float32)
  if n == 1:
    mask[:] = 1
  w = rs.choice([-0.5, -0.25, 0.25, 0.5, 1.0], size=n).astype(np.float32)
  g = rs.choice([0.0, 0.125, -0.125, 0.75], size=n).astype(np.float32)
  mom = rs.choice([-1.0, 0.5, 2.0], size=n).astype(np.float32)
  return mask, w, g, mom


def _k2_bytes(ns):
  from rigl_amd import _lib
  return int(_lib.load().rigl_prune_regrow_workspace_bytes((C.c_int64 * len(ns))(*ns), len(ns)))


@pytest.mark.parametrize('n', K2_SIZES)
def test_prune_regrow_single_layer(n):
  from rigl_amd import ops
  mask, w, g, mom = _k2_data(n, n)
  ref = O.rigl_mask_update(mask, w, g, 0.3, momentum=mom)

  def body():
    nm, nw, nmom, counts = TK._run_rigl(ops, mask, w, g, 0.3, mom=mom)
    TK._diff('mask', nm, ref['mask'])
    TK._diff('weights', nw, ref['weights'])
    TK._diff('momentum', nmom, ref['momentum'])
    assert (counts[0], counts[1], counts[2]) == (ref['n_ones'], ref['n_prune'], ref['n_keep'])
    return nm, nw, nmom, counts
  _both_poisons('prune_regrow n=%d' % n, body, want_bytes=_k2_bytes([n]))


def test_prune_regrow_batched_over_every_size_in_both_orders():
  """One call over all six sizes ascending and then descending: the layout's regions are sums over the layers."""
  from rigl_amd import ops
  sizes = list(K2_SIZES) + list(reversed(K2_SIZES))
  data = [_k2_data(n, 100 + i) for i, n in enumerate(sizes)]
  refs = [O.rigl_mask_update(m, w, g, 0.3, momentum=mom) for m, w, g, mom in data]

  def body():
    layers = [dict(w=TK._t(w), momentum=TK._t(mom), mask_bits=ops.mask_pack(TK._t(m)), dense_grad=TK._t(g))
              for m, w, g, mom in data]
    counts = ops.prune_regrow(layers, 0.3).cpu().numpy()
    out = [counts]
    for i, (n, l, ref) in enumerate(zip(sizes, layers, refs)):
      what = 'layer %d (n=%d) ' % (i, n)
      nm = ops.mask_unpack(l['mask_bits'], (n,)).cpu().numpy()
      TK._diff(what + 'mask', nm, ref['mask'])
      TK._diff(what + 'weights', l['w'].cpu().numpy(), ref['weights'])
      TK._diff(what + 'momentum', l['momentum'].cpu().numpy(), ref['momentum'])
      assert (counts[i][0], counts[i][1], counts[i][2]) == (ref['n_ones'], ref['n_prune'], ref['n_keep']), what
      out += [nm, l['w'], l['momentum']]
    return out
  _both_poisons('prune_regrow batched x%d' % len(sizes), body, want_bytes=_k2_bytes(sizes))


@pytest.mark.parametrize('n', [33, 4097, 70001])
def test_prune_regrow_selections(n):
  from rigl_amd import _lib, ops
  mask, w, g, _ = _k2_data(n, n + 1)
  need = int(_lib.load().rigl_prune_regrow_selections_workspace_bytes(n))

  def body():
    ref = TK._check_selections(ops, 'ties n=%d' % n, mask, w, g, 0.3, None, None, 'zeros', 0.0)
    return ref['mask'], ref['weights']
  _both_poisons('prune_regrow_selections n=%d' % n, body, want_bytes=need)


def test_prune_regrow_two_slot_forms():
  """rigl_prune_regrow_slots and rigl_prune_regrow_selections_slots: the second optimizer slot is reset like the first, so
  each slot is the oracle's momentum of a run that carried it."""
  from rigl_amd import _lib, ops
  n = 4097
  mask, w, g, mom = _k2_data(n, 7)
  mom2 = np.abs(_k2_data(n, 8)[3])
  ref = O.rigl_mask_update(mask, w, g, 0.3, momentum=mom, initial_acc_scale=0.5)
  ref2 = O.rigl_mask_update(mask, w, g, 0.3, momentum=mom2, initial_acc_scale=0.5)

  def body():
    outs = []
    for sel in (False, True):
      l = dict(w=TK._t(w), momentum=TK._t(mom), momentum2=TK._t(mom2), mask_bits=ops.mask_pack(TK._t(mask)), dense_grad=TK._t(g))
      if sel:
        ops.prune_regrow_selections(l, 0.3, initial_acc_scale=0.5, want_indices=False)
      else:
        ops.prune_regrow([l], 0.3, initial_acc_scale=0.5)
      what = 'two slots%s ' % (' (selections)' if sel else '')
      nm = ops.mask_unpack(l['mask_bits'], (n,)).cpu().numpy()
      TK._diff(what + 'mask', nm, ref['mask'])
      TK._diff(what + 'weights', l['w'].cpu().numpy(), ref['weights'])
      TK._diff(what + 'slot 1', l['momentum'].cpu().numpy(), ref['momentum'])
      TK._diff(what + 'slot 2', l['momentum2'].cpu().numpy(), ref2['momentum'])
      outs += [nm, l['w'], l['momentum'], l['momentum2']]
    return outs
  log = _both_poisons('prune_regrow two slots n=%d' % n, body)
  assert [b for _, b, _ in log] == [_k2_bytes([n]), int(_lib.load().rigl_prune_regrow_selections_workspace_bytes(n))]


def test_topk_mask_single_and_batched():
  """ops.topk_mask per size and ops.topk_mask_batched over all of them in both orders, against oracle topk_order (ties:
  lower index first), the mask words starting from a sentinel."""
  from rigl_amd import ops
  sizes = list(K2_SIZES) + list(reversed(K2_SIZES))
  rs = np.random.RandomState(3)
  items = [((rs.randint(0, 50, size=n) / 7.0).astype(np.float32), int(n * f)) for n, f in zip(sizes, (1.0, .3, .5, .25, .75, .1) * 2)]
  refs = []
  for s, k in items:
    r = np.zeros(s.size, np.float32)
    r[O.topk_order(s)[:k]] = 1
    refs.append(r)

  def body():
    mk = lambda s: torch.full((ops.n_mask_words(s.size),), 0x5A5A5A5A, dtype=torch.int32, device=DEV)   # noqa: E731
    alone = [ops.topk_mask(TK._t(s), k, out=mk(s)) for s, k in items]
    batch = [(TK._t(s), k, mk(s)) for s, k in items]
    ops.topk_mask_batched(batch)
    for i, ((s, k), one, (_, _, bits), ref) in enumerate(zip(items, alone, batch, refs)):
      TK._diff('topk n=%d k=%d' % (s.size, k), ops.mask_unpack(one, (s.size,)).cpu().numpy(), ref)
      assert torch.equal(one, bits), 'layer %d: the batched call is not the words of its own call' % i
    return alone
  log = _both_poisons('topk_mask', body)
  assert [b for _, b, _ in log] == [_k2_bytes([n]) for n in sizes] + [_k2_bytes(sizes)]


def test_magnitude_prune_batched():
  """contrib model_pruning's threshold update over the six sizes in one call, against tests/prune_ref.py (the NumPy
  restatement the golden cases pin): threshold bits, bitmap, counts; weights untouched."""
  from rigl_amd import _lib, ops
  rs = np.random.RandomState(9)
  ws = [(rs.randint(-8, 9, size=n) / 16.0).astype(np.float32) for n in K2_SIZES]       # heavy ties in |w|
  ks = [max(1, int(n * 0.4)) for n in K2_SIZES]
  thr0 = [0.01 * i for i in range(len(ws))]
  refs = [prune_ref.mask_update(w, k, t, 0.5) for w, k, t in zip(ws, ks, thr0)]
  need = int(_lib.load().rigl_magnitude_prune_batched_workspace_bytes(len(ws)))

  def body():
    items = [(TK._t(w), torch.zeros((w.size + 31) // 32, dtype=torch.int32, device=DEV),
              torch.full((1,), t, dtype=torch.float32, device=DEV), k) for w, k, t in zip(ws, ks, thr0)]
    counts = torch.full((len(items), 4), -1, dtype=torch.int32, device=DEV)
    ops.magnitude_prune_batched(items, 0.5, counts)
    cn = counts.cpu().numpy()
    for i, ((w, bits, thr, k), (t_ref, m_ref)) in enumerate(zip(items, refs)):
      assert thr.cpu().numpy().view(np.uint32)[0] == np.float32(t_ref).view(np.uint32), 'layer %d: threshold bits' % i
      np.testing.assert_array_equal(bits.cpu().numpy().view(np.uint32), prune_ref.pack_bits(m_ref), err_msg='layer %d' % i)
      assert (cn[i, 0], cn[i, 1], cn[i, 2]) == (w.numel(), k, int(m_ref.sum())), 'layer %d: counts' % i
      assert torch.equal(w.cpu(), torch.from_numpy(ws[i])), 'layer %d: weights changed' % i
    return [counts] + [it[1] for it in items] + [it[2] for it in items]
  _both_poisons('magnitude_prune_batched', body, want_bytes=need)


# ---------------------------------------------------------------------------------------------------------------------
# the K-split forward: chosen from workspace_bytes
# ---------------------------------------------------------------------------------------------------------------------
def test_conv_fwd_with_a_ksplit_plan_and_no_workspace():
  """fwd_impl (conv.hip) takes the K-split plan of an ordinary layer only when ``workspace && workspace_bytes >= need``
  (the line under plan_pp<0>) and otherwise "runs unsplit": the split is decided by workspace_bytes, so a caller that
  brings none must still get the layer's bits.  PP_CASES' 36-K-tile 3x3 layer (five 128-row tiles: few enough to split)
  with "pp_ksplit_min_kt" lowered to 32 so that the plan exists at this size: a direct library call with a ZERO-LENGTH
  guarded workspace, and the same call with the exactly-sized one, must both give exactref's expected bits -- exact for any
  summation order, so split and unsplit agree -- and neither may touch a guard."""
  from rigl_amd import _lib, ops
  lib = _lib.load()
  case = k1_check.PP_CASES[10]
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  assert (k * k * Cin // 64, Cin, Cout) == (36, 256, 256)
  d = ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo)
  g = _guard()
  ops.tune_set('pp_ksplit_min_kt', 32)
  try:
    need = int(lib.rigl_conv2d_workspace_bytes(C.byref(d), 0))
    assert need > 0, 'the layer has no K-split plan here: the case would not reach the branch'
    for regime in ('low', 'round'):
      op = E.operands(case, 110, regime, DEV)
      x = op.x.to(torch.bfloat16)
      ohwi = torch.empty(op.w.numel(), dtype=torch.bfloat16, device=DEV)
      ops.pack_weights(op.w.reshape(-1).contiguous(), None, k * k * Cin, Cout, None, ohwi)
      ref, ab = E.reference(op, ('y',))
      E.check_conditions(op, ref, ab)
      want = E.expect_plain(ref['y'])
      for p in G.POISONS:
        g.poison = p
        for nbytes in (0, need):
          ws = g(nbytes, DEV, 'ksplit')
          assert ws.numel() == nbytes
          y, chk, _ = E.guarded((N, Ho, Wo, Cout), torch.bfloat16, DEV)
          _lib.check(lib.rigl_masked_conv2d_fwd(C.byref(d), ops._ptr(x), ops._ptr(ohwi), ops._ptr(y), ops._ptr(ws), nbytes,
                                                ops._stream()))
          what = 'fwd %s workspace %d of %d bytes, poison 0x%02X' % (regime, nbytes, need, p)
          chk(what)
          E.assert_bits(what, E.got_bits(y), want)
          log = g.check(what)
          print('workspace %s: %s' % (what, [list(l) for l in log]))
          assert log[0][2] == 0 or nbytes == need        # (nothing to write into a zero-length payload)
  finally:
    ops.tune_unset('pp_ksplit_min_kt')
    g.check('after the K-split case')


def test_bwd_grid_with_a_workspace():
  """rigl_masked_conv2d_bwd_grid is the one K1 form whose cases in the nine small sets are all too short for a split weight
  gradient (no workspace, nothing to guard): tests/k1_exact.py's own walk of one strided 1x1 layer with 1 024 output rows,
  every form of the conv on the guarded workspace with the expected bits of tests/exactref.py, both regimes, both poisons."""
  from tests import k1_exact as K
  g = _guard()
  K.WS.guard, K.WS.poisons, K.WS.by_form = g, G.POISONS, {}
  try:
    with G.installed(g):
      for regime in ('low', 'round'):
        K.run_conv_case(GRID, 100, regime, [{}])
        K._ws_check('end of the case')
    forms = dict(K.WS.by_form)
  finally:
    K.WS.guard, K.WS.poisons, K.WS.by_form = None, (), {}
    g.check('after the bwd_grid case')
  print('workspace bwd_grid case %s: %s' % (GRID, forms))
  assert forms['bwd_grid.dx'][0] == 4 and forms['bwd_grid.dx'][1] > 0, 'the grid form ran without a workspace'


# ---------------------------------------------------------------------------------------------------------------------
# the error contract, host side only
# ---------------------------------------------------------------------------------------------------------------------
class _Bufs:
  """Device buffers of one refused call: inputs (zeros: they are never read) and sentinel-filled outputs."""
  FILL = 0x5A

  def __init__(self):
    self.keep, self.outs = [], []

  def inp(self, nbytes):
    self.keep.append(torch.zeros(max(int(nbytes), 1), dtype=torch.uint8, device=DEV))
    return self.keep[-1].data_ptr()

  def out(self, nbytes):
    self.outs.append(torch.full((max(int(nbytes), 1),), self.FILL, dtype=torch.uint8, device=DEV))
    return self.outs[-1].data_ptr()


def _desc(case):
  from rigl_amd import ops
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  return ops.conv_desc(N, H, W, Cin, Cout, k, k, stride, pt, pl, Ho, Wo)


def _conv_sizes(case):
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  return N * H * W * Cin, N * Ho * Wo * Cout, k * k * Cin * Cout


ORDINARY = (4, 16, 16, 64, 128, 3, 1, 1, 1, 16, 16)          # the shared igemm launch, a split-K weight gradient
SLICED = (8, 64, 64, 128, 128, 1, 1, 0, 0, 64, 64)           # bwdslice.hpp: the layers that take a masked addend
BNA = (16, 64, 64, 64, 256, 1, 1, 0, 0, 64, 64)              # bwd1x1.hpp with the batch norm's backward on load
SMALL_CIN = (3, 9, 11, 20, 40, 3, 1, 1, 1, 9, 11)            # the im2col repack in front of the forward
TINY_CIN = (2, 16, 16, 3, 16, 3, 1, 1, 1, 16, 16)            # the padded 4-channel copy
F32 = (2, 224, 224, 3, 64, 7, 2, 3, 3, 112, 112)
DEPTHWISE = (2, 16, 16, 32, 32, 3, 1, 1, 1, 16, 16)
BN_M, BN_C = 1000, 64
POOL = GR.small_pool_geometries()[0][1]
K2_N = 4097


def _conv_call(name, case, which):
  """(need, call(bufs, ws, nbytes) -> rc) of one conv entry point; ``which`` = the rigl_conv2d_workspace_bytes selector."""
  from rigl_amd import _lib, ops
  lib = _lib.load()
  d = _desc(case)
  nx, ny, nw = _conv_sizes(case)
  N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo = case
  st = ops._stream()
  need = int(lib.rigl_conv2d_workspace_bytes(C.byref(d), which))
  x, dy, w = (lambda b: b.inp(nx * 2)), (lambda b: b.inp(ny * 2)), (lambda b: b.inp(nw * 2))
  dw, dx, y = (lambda b: b.out(nw * 4)), (lambda b: b.out(nx * 2)), (lambda b: b.out(ny * 2))
  calls = {
      'rigl_masked_conv2d_fwd': lambda b, ws, n: lib.rigl_masked_conv2d_fwd(C.byref(d), x(b), w(b), y(b), ws, n, st),
      'rigl_masked_conv2d_fwd_stats': lambda b, ws, n: lib.rigl_masked_conv2d_fwd_stats(
          C.byref(d), x(b), w(b), y(b), b.out(lib.rigl_conv2d_stats_parts(C.byref(d)) * 2 * Cout * 4),
          lib.rigl_conv2d_stats_parts(C.byref(d)) * 2 * Cout, ws, n, st),
      'rigl_masked_conv2d_fwd_relu': lambda b, ws, n: lib.rigl_masked_conv2d_fwd_relu(C.byref(d), x(b), w(b), y(b), ws, n, st),
      'rigl_masked_conv2d_wgrad': lambda b, ws, n: lib.rigl_masked_conv2d_wgrad(C.byref(d), x(b), dy(b), dw(b), ws, n, st),
      'rigl_masked_conv2d_bwd': lambda b, ws, n: lib.rigl_masked_conv2d_bwd(
          C.byref(d), x(b), dy(b), w(b), b.inp(nx * 2), dw(b), dx(b), ws, n, st),
      'rigl_masked_conv2d_bwd_sub': lambda b, ws, n: lib.rigl_masked_conv2d_bwd_sub(
          C.byref(d), x(b), dy(b), w(b), b.inp(nx * 2), 2, 2, dw(b), dx(b), ws, n, st),
      'rigl_masked_conv2d_bwd_relu': lambda b, ws, n: lib.rigl_masked_conv2d_bwd_relu(
          C.byref(d), x(b), dy(b), w(b), dw(b), dx(b), ws, n, st),
      'rigl_masked_conv2d_bwd_grid': lambda b, ws, n: lib.rigl_masked_conv2d_bwd_grid(
          C.byref(d), x(b), dy(b), w(b), dw(b), b.out(N * Ho * Wo * Cin * 2), ws, n, st),
      'rigl_masked_conv2d_bwd_masked': lambda b, ws, n: lib.rigl_masked_conv2d_bwd_masked(
          C.byref(d), x(b), dy(b), w(b), b.inp(nx * 2), b.inp(nx // 8), dw(b), dx(b), ws, n, st),
      'rigl_masked_conv2d_bwd_bnapply': lambda b, ws, n: lib.rigl_masked_conv2d_bwd_bnapply(
          C.byref(d), x(b), dy(b), w(b), None, dw(b), dx(b), ws, n, b.inp(ny * 2), b.inp(ny // 8), b.inp(Cout * 4),
          b.inp(Cout * 4), b.inp(3 * Cout * 4), st),
      'rigl_masked_conv2d_wgrad_f32': lambda b, ws, n: lib.rigl_masked_conv2d_wgrad_f32(
          C.byref(d), b.inp(nx * 4), b.inp(ny * 4), dw(b), ws, n, st),
      'rigl_depthwise_conv2d_wgrad': lambda b, ws, n: lib.rigl_depthwise_conv2d_wgrad(
          C.byref(d), x(b), dy(b), b.out(k * k * Cin * 4), ws, n, st),
  }
  if name == 'rigl_masked_conv2d_wgrad_f32':
    need = int(lib.rigl_conv2d_wgrad_f32_workspace_bytes(C.byref(d)))
  if name == 'rigl_depthwise_conv2d_wgrad':
    need = int(lib.rigl_depthwise_conv2d_workspace_bytes(C.byref(d)))
  return need, calls[name]


def _bn_call(name):
  from rigl_amd import _lib, ops
  lib = _lib.load()
  m, c, st = BN_M, BN_C, ops._stream()
  t = lambda b: b.inp(m * c * 2)            # noqa: E731  a bf16 [m, c] input
  o = lambda b: b.out(m * c * 2)            # noqa: E731  ... output
  v = lambda b: b.inp(c * 4)                # noqa: E731  an fp32 [c] input
  r = lambda b: b.out(c * 4)                # noqa: E731  ... output
  need = int(lib.rigl_bn_workspace_bytes(m, c))
  calls = {
      # bn.hip fwd_statistics: the check is its first statement without producer partials, before k_reduce
      'rigl_bn_fwd': lambda b, ws, n: lib.rigl_bn_fwd(m, c, t(b), None, v(b), v(b), r(b), r(b), 0.1, 1e-5, 1, o(b), r(b), r(b), r(b),
                                                      r(b), ws, n, st),
      'rigl_bn_fwd_stats': lambda b, ws, n: lib.rigl_bn_fwd_stats(m, c, t(b), None, v(b), v(b), r(b), r(b), 0.1, 1e-5, 1, o(b), r(b),
                                                                  r(b), r(b), r(b), None, 0, b.out(m * c // 8), ws, n, st),
      'rigl_bn_fwd_statistics': lambda b, ws, n: lib.rigl_bn_fwd_statistics(m, c, t(b), v(b), v(b), r(b), r(b), 0.1, 1e-5, r(b), r(b),
                                                                            r(b), r(b), None, 0, ws, n, st),
      'rigl_bn_add_bn_fwd': lambda b, ws, n: lib.rigl_bn_add_bn_fwd(m, c, t(b), t(b), v(b), v(b), v(b), v(b), r(b), r(b), 0.1, 1e-5, 1,
                                                                    o(b), r(b), r(b), r(b), r(b), None, 0, b.out(m * c // 8), ws, n, st),
      # bn.hip bn_bwd_impl: the check follows the argument checks and precedes make_geom and every launch
      'rigl_bn_bwd': lambda b, ws, n: lib.rigl_bn_bwd(m, c, t(b), None, b.inp(m * c // 8), t(b), v(b), v(b), v(b), v(b), v(b), 1, o(b),
                                                      o(b), r(b), r(b), ws, n, st),
      'rigl_bn_bwd_reduce': lambda b, ws, n: lib.rigl_bn_bwd_reduce(m, c, t(b), b.inp(m * c // 8), t(b), v(b), v(b), v(b), 1, r(b), r(b),
                                                                    b.out(3 * c * 4), ws, n, st),
  }
  if name == 'rigl_bn_add_bn_bwd':          # bn.hip rigl_bn_add_bn_bwd: the check precedes the LDS opt-in and the three launches
    need = int(lib.rigl_bn_add_bn_bwd_workspace_bytes(m, c))
    return need, lambda b, ws, n: lib.rigl_bn_add_bn_bwd(m, c, t(b), t(b), b.inp(m * c // 8), t(b), v(b), v(b), v(b), v(b), v(b), v(b),
                                                         o(b), o(b), r(b), r(b), r(b), r(b), ws, n, st)
  if name == 'rigl_bn_relu_maxpool_bwd':    # pool.hip: the check follows the NULL checks and precedes k_bn_relu_bwd<0>
    from tests import test_glue_edges_gpu as TG
    gd = TG._gdesc(POOL)
    nin, nout, pc = POOL.n * POOL.h * POOL.w * POOL.cin, POOL.n * POOL.ho * POOL.wo * POOL.cin, POOL.cin
    need = int(lib.rigl_bn_relu_maxpool_bwd_workspace_bytes(C.byref(gd)))
    return need, lambda b, ws, n: lib.rigl_bn_relu_maxpool_bwd(
        C.byref(gd), b.inp(nin * 2), b.inp(nout * 2), b.inp(nout), b.inp(pc * 4), b.inp(pc * 4), b.inp(pc * 4), b.inp(pc * 4),
        b.inp(pc * 4), b.out(nin * 2), b.out(pc * 4), b.out(pc * 4), ws, n, st)
  return need, calls[name]


def _k2_call(name):
  from rigl_amd import _lib, ops
  lib = _lib.load()
  n, st = K2_N, ops._stream()
  words = (n + 31) // 32
  prm = _lib.PruneRegrowParams(0.3, _lib.GROW_ZEROS, 1.0, _lib.MOMRESET_GRAD, 0.0, 0)

  def layer(b):                              # w, momentum and the bitmap are updated in place: outputs here
    l = _lib.PruneRegrowLayer()
    l.n, l.w, l.momentum, l.mask_bits, l.dense_grad = n, b.out(n * 4), b.out(n * 4), b.out(words * 4), b.inp(n * 4)
    return l
  need = _k2_bytes([n])
  # prune_regrow.hip run(): the check follows the per-layer argument checks and precedes k_write_table, the first launch
  if name == 'rigl_prune_regrow':
    return need, lambda b, ws, nb: lib.rigl_prune_regrow(C.byref(layer(b)), 1, C.byref(prm), b.out(32), ws, nb, st)
  if name == 'rigl_prune_regrow_slots':
    return need, lambda b, ws, nb: lib.rigl_prune_regrow_slots(C.byref(layer(b)), (C.c_void_p * 1)(b.out(n * 4)), 1, C.byref(prm),
                                                               b.out(32), ws, nb, st)
  if name == 'rigl_topk_mask':
    return need, lambda b, ws, nb: lib.rigl_topk_mask(b.inp(n * 4), n, n // 3, b.out(words * 4), ws, nb, st)
  if name == 'rigl_topk_mask_batched':
    def call(b, ws, nb):
      t = _lib.TopkLayer()
      t.score, t.n, t.n_keep, t.mask_bits = b.inp(n * 4), n, n // 3, b.out(words * 4)
      return lib.rigl_topk_mask_batched(C.byref(t), 1, ws, nb, st)
    return need, call
  if name == 'rigl_magnitude_prune_batched':   # run_mag(): after the per-layer checks, before k_write_table
    def call(b, ws, nb):
      t = _lib.MagnitudePruneLayer()
      t.n, t.w, t.mask_bits, t.threshold, t.k = n, b.inp(n * 4), b.out(words * 4), b.out(4), n // 3
      return lib.rigl_magnitude_prune_batched(C.byref(t), 1, 0.5, b.out(16), ws, nb, st)
    return int(lib.rigl_magnitude_prune_batched_workspace_bytes(1)), call
  # rigl_prune_regrow_selections_slots: the check follows the argument checks and precedes run() and the sorts
  need = int(lib.rigl_prune_regrow_selections_workspace_bytes(n))
  if name == 'rigl_prune_regrow_selections':
    return need, lambda b, ws, nb: lib.rigl_prune_regrow_selections(
        C.byref(layer(b)), C.byref(prm), b.out(words * 4), b.out(words * 4), b.out(n * 4), b.out(n * 4), b.out(32), ws, nb, st)
  assert name == 'rigl_prune_regrow_selections_slots'
  return need, lambda b, ws, nb: lib.rigl_prune_regrow_selections_slots(
      C.byref(layer(b)), b.out(n * 4), C.byref(prm), b.out(words * 4), b.out(words * 4), b.out(n * 4), b.out(n * 4), b.out(32), ws, nb, st)


# entry point -> how its (need, call) is made.  The size check of each was read in the source: conv.hip fwd_impl (tiny- / small-
# Cin layers only: after the argument checks, before k_pad_input4 / k_im2col), wgrad_impl (the body of rigl_masked_conv2d_wgrad:
# before its first launch), bwd_impl (at the head of each path that launches itself -- bwd1x1, bwdslice and the two shared
# launches --, before that path's launch; the row-streaming and c3x3 paths and the two-launch tail go through wgrad_impl),
# rigl_masked_conv2d_bwd_bnapply, conv_f32.hip, depthwise.hip (each right after the NULL checks).
REFUSALS = [
    ('rigl_masked_conv2d_fwd', lambda n: _conv_call(n, SMALL_CIN, 0)),
    ('rigl_masked_conv2d_fwd_stats', lambda n: _conv_call(n, TINY_CIN, 0)),
    ('rigl_masked_conv2d_fwd_relu', lambda n: _conv_call(n, SMALL_CIN, 0)),
    ('rigl_masked_conv2d_wgrad', lambda n: _conv_call(n, ORDINARY, 2)),
    ('rigl_masked_conv2d_bwd', lambda n: _conv_call(n, ORDINARY, 2)),
    ('rigl_masked_conv2d_bwd_sub', lambda n: _conv_call(n, ORDINARY, 2)),
    ('rigl_masked_conv2d_bwd_relu', lambda n: _conv_call(n, ORDINARY, 2)),
    ('rigl_masked_conv2d_bwd_grid', lambda n: _conv_call(n, GRID, 2)),
    ('rigl_masked_conv2d_bwd_masked', lambda n: _conv_call(n, SLICED, 2)),
    ('rigl_masked_conv2d_bwd_bnapply', lambda n: _conv_call(n, BNA, 2)),
    ('rigl_masked_conv2d_wgrad_f32', lambda n: _conv_call(n, F32, 2)),
    ('rigl_depthwise_conv2d_wgrad', lambda n: _conv_call(n, DEPTHWISE, 2)),
    ('rigl_bn_fwd', _bn_call), ('rigl_bn_fwd_stats', _bn_call), ('rigl_bn_fwd_statistics', _bn_call),
    ('rigl_bn_add_bn_fwd', _bn_call), ('rigl_bn_bwd', _bn_call), ('rigl_bn_bwd_reduce', _bn_call),
    ('rigl_bn_add_bn_bwd', _bn_call), ('rigl_bn_relu_maxpool_bwd', _bn_call),
    ('rigl_prune_regrow', _k2_call), ('rigl_prune_regrow_slots', _k2_call), ('rigl_prune_regrow_selections', _k2_call),
    ('rigl_prune_regrow_selections_slots', _k2_call), ('rigl_topk_mask', _k2_call), ('rigl_topk_mask_batched', _k2_call),
    ('rigl_magnitude_prune_batched', _k2_call),
]
# Taken with a workspace argument that the library does not use (include/rigl_hip.h says so at each): nothing to refuse.
IGNORED = ('rigl_masked_conv2d_dgrad', 'rigl_masked_conv2d_dgrad_acc', 'rigl_masked_conv2d_fwd_bnrelu')


def test_the_lists_cover_every_entry_point_of_the_header_that_takes_a_workspace():
  import os
  import re
  text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'rigl_hip.h')).read()
  text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
  takes = {m.group(1) for m in re.finditer(r'\bint\s+(rigl_\w+)\s*\(([^;]*?)\)\s*;', text, flags=re.S)
           if re.search(r'\bworkspace_bytes\b', m.group(2))}
  assert len(takes) == 30
  assert takes == {r[0] for r in REFUSALS} | set(IGNORED)


@pytest.mark.parametrize('name,make', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_a_short_or_missing_workspace_is_refused_before_anything_is_launched(name, make):
  from rigl_amd import _lib
  need, call = make(name)
  assert need > 0, name + ': the query is 0 at this shape, nothing to refuse'
  # (the buffer holds all `need` bytes: the call only CLAIMS one byte less)
  ws = torch.full((need,), _Bufs.FILL, dtype=torch.uint8, device=DEV)
  bufs = []
  for what, ptr, nbytes in (('need - 1', ws.data_ptr(), need - 1), ('NULL', None, need)):
    b = _Bufs()
    rc = call(b, ptr, nbytes)
    assert rc == _lib.RIGL_EWORKSPACE, '%s with workspace %s: returned %d (%s), not RIGL_EWORKSPACE' % (
        name, what, rc, _lib.load().rigl_last_error().decode('utf-8', 'replace'))
    bufs.append(b)
  torch.cuda.synchronize()
  for b in bufs:
    for o in b.outs:
      assert bool((o == _Bufs.FILL).all()), name + ': an output was written by a refused call'
  assert bool((ws == _Bufs.FILL).all()), name + ': the workspace was written by a refused call'
