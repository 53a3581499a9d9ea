"""rigl_summary_step on the GPU against tests/summary_ref.py: the edge shapes, masks and data of ``summary_ref.tables()``,
integer outputs exact, every finite fp64 sum within 2 * n * 2^-53 * S_ref (all terms are non-negative and exact in fp64, so any
summation order in fp64 stays inside it), non-finite sums of the reference's class; the bits independent of the grid, of the
run and of what the workspace held; refusals that touch nothing; the ring read back through TrainingSummaries.read()."""
import ctypes as C
import math

import numpy as np
import pytest

import summary_ref as R
import wsguard

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
F32 = np.float32
GUARD = 4096


@pytest.fixture(scope='module')
def cases():
  """[(table, per-entry reference, totals reference)], computed once and never modified."""
  return [(t,) + R.table_sums(t) for t in R.tables()]


class Device:
  """A table of summary_ref.tables() on the device, with a guarded ring and a guarded step counter."""

  def __init__(self, table, ring_slots=3, step0=0):
    from rigl_amd import ops
    self.W = torch.from_numpy(table['W']).to(DEV)
    self.G = torch.from_numpy(table['G']).to(DEV)
    self.B = torch.from_numpy(table['B'].view(np.int32)).to(DEV)
    rows = []
    for e in table['entries']:
      o, n = e['offset'], e['n']
      bits = self.B[o // 32:o // 32 + (n + 31) // 32] if e['has_mask'] else None
      rows.append((self.W[o:o + n], self.G[o:o + n], bits, e['weight_decay'], e['apply_mask']))
    self.rows = rows
    self.table = ops.summary_table(rows)
    self.n_entries = len(rows)
    self.grad_scale = table['grad_scale']
    self.slots = ring_slots
    self.slot_bytes = ops.summary_slot_bytes(self.n_entries)
    self.buf = torch.full((GUARD + ring_slots * self.slot_bytes + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    self.ring = self.buf[GUARD:GUARD + ring_slots * self.slot_bytes]
    self.counter = torch.tensor([-7, step0, -9], dtype=torch.int32, device=DEV)
    self.step = self.counter[1:2]
    self.loss = torch.tensor([1.25], dtype=torch.float32, device=DEV)

  def run(self, max_blocks=0, lr=0.1, lr_device=None, loss=True):
    from rigl_amd import ops
    ops.summary_step(self.table, self.step, self.ring, self.slots, grad_scale=self.grad_scale,
                     loss=self.loss if loss else None, lr=lr if lr_device is None else None, lr_device=lr_device,
                     max_blocks=max_blocks)

  def state(self):
    torch.cuda.synchronize()
    return self.buf.cpu().numpy().copy(), self.counter.cpu().numpy().copy()

  def slot(self, k):
    host = self.ring.cpu().numpy()
    return host[k * self.slot_bytes:(k + 1) * self.slot_bytes].copy()


def _check(rec, table, ent, tot):
  ns = [e['n'] for e in table['entries']]
  for k in R.COUNT_FIELDS:
    assert rec['entries'][k].tolist() == ent[k], k
    assert rec['totals'][k] == tot[k], k
  for k in R.FLOAT_FIELDS:
    for i, (got, ref, n) in enumerate(zip(rec['entries'][k].tolist(), ent[k], ns)):
      assert R.float_ok(got, ref, max(n, 1)), (table['name'], k, i, n, got, ref, R.bound(max(n, 1), ref))
    assert R.float_ok(rec['totals'][k], tot[k], max(sum(ns), 1)), (table['name'], k, rec['totals'][k], tot[k])


def test_every_case_matches_the_reference(cases):
  from rigl_amd import summaries as S
  for table, ent, tot in cases:
    d = Device(table, step0=4)
    before = d.state()
    d.run()
    buf, counter = d.state()
    assert counter.tolist() == [-7, 5, -9]
    assert (buf[:GUARD] == 0xA5).all() and (buf[-GUARD:] == 0xA5).all()
    ring = buf[GUARD:-GUARD].reshape(3, d.slot_bytes)
    assert (ring[0] == 0xA5).all() and (ring[2] == 0xA5).all()             # slot 4 % 3 == 1 and no other
    assert (before[0] == 0xA5).all()
    rec = S.parse_slot(ring[1], d.n_entries)
    assert rec['step'] == 4 and rec['n_entries'] == d.n_entries
    assert rec['loss'] == 1.25 and rec['learning_rate'] == float(F32(0.1))
    _check(rec, table, ent, tot)
    if table['name'] == 'nonfinite':                                        # the reference itself: a blown-up step shows
      assert math.isnan(tot['sumsq_g']) and tot['nonfinite_g'] >= 8 and math.isnan(tot['sumsq_w'])
      assert ent['sumsq_g'][0] < math.inf and ent['nonfinite_g'][0] == 0   # masked-off inf: a zero
      assert ent['sumsq_g'][3] == math.inf and ent['nonfinite_g'][3] == 1  # masked-on inf


def test_bits_do_not_depend_on_the_grid_the_run_or_the_workspace(cases):
  for table, _, _ in cases:
    d = Device(table, ring_slots=1)
    outs = []
    for mb in (0, 1, 7, 0):
      d.run(max_blocks=mb)
      torch.cuda.synchronize()
      outs.append(d.slot(0))
    for poison in wsguard.POISONS:
      g = wsguard.GuardedWorkspace(poison=poison)
      with wsguard.installed(g):
        d.run()
        log = g.check('summary_step')                                       # the guards around the exact-size payload are intact
      from rigl_amd import ops
      assert [(tag, nbytes) for tag, nbytes, _ in log] == [('summary', ops.summary_workspace_bytes(d.table))]
      outs.append(d.slot(0))
    head = outs[0][:4].view(np.int32)[0]
    for k, o in enumerate(outs):
      assert o[:4].view(np.int32)[0] == head + k                            # the step moves on ...
      np.testing.assert_array_equal(o[4:], outs[0][4:])                     # ... and nothing else differs in any bit


def test_rate_from_a_device_pointer_and_no_loss(cases):
  from rigl_amd import summaries as S
  table = cases[0][0]
  d = Device(table, ring_slots=2, step0=-3)                                  # a wrapped (negative) counter: slot (-3) mod 2 == 1
  rate = torch.tensor([0.0625], dtype=torch.float32, device=DEV)
  d.run(lr_device=rate, loss=False)
  torch.cuda.synchronize()
  rec = S.parse_slot(d.slot(1), d.n_entries)
  assert rec['step'] == -3 and rec['learning_rate'] == 0.0625 and math.isnan(rec['loss'])
  assert int(d.step.cpu()[0]) == -2


def test_refusals_write_nothing(cases):
  from rigl_amd import _lib, ops
  table = cases[0][0]
  d = Device(table)
  lib = _lib.load()
  arr, n = d.table
  need = ops.summary_workspace_bytes(d.table)
  assert need == lib.rigl_summary_workspace_bytes(arr, n) > 0
  ws = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device=DEV)
  assert ws.data_ptr() % 256 == 0
  before = d.state()
  ws_before = ws.cpu().numpy().copy()
  stream = ops._stream()

  def call(tab, ring_slots=3, wsp=ws.data_ptr(), ws_bytes=need):
    return lib.rigl_summary_step(tab, n, 0.3, C.c_void_p(d.loss.data_ptr()), None, 0.1, C.c_void_p(d.step.data_ptr()),
                                 C.c_void_p(d.ring.data_ptr()), ring_slots, C.c_void_p(wsp) if wsp else None, ws_bytes, 0, stream)
  assert call(arr, ws_bytes=need - 1) == _lib.RIGL_EWORKSPACE
  assert call(arr, wsp=0) == _lib.RIGL_EWORKSPACE
  assert call(arr, ring_slots=0) == _lib.RIGL_EINVAL
  assert call(arr, ring_slots=-1) == _lib.RIGL_EINVAL
  big = next(i for i, e in enumerate(table['entries']) if e['n'] >= 64 and e['has_mask'])
  for field, delta, what in (('w', 4, b'16-byte'), ('g', 8, b'16-byte'), ('mask_bits', 2, b'mask_bits')):
    bad = (_lib.SummaryEntry * n)()
    C.memmove(bad, arr, C.sizeof(bad))
    setattr(bad[big], field, getattr(bad[big], field) + delta)
    assert call(bad) == _lib.RIGL_EINVAL
    assert what in lib.rigl_last_error()
  after = d.state()
  np.testing.assert_array_equal(before[0], after[0])                        # the ring and the guard bytes around it
  np.testing.assert_array_equal(before[1], after[1])                        # the counter and its neighbours
  np.testing.assert_array_equal(ws_before, ws.cpu().numpy())
  assert call(arr) == _lib.RIGL_OK                                           # and the same arguments, unbroken, are accepted
  torch.cuda.synchronize()
  assert int(d.step.cpu()[0]) == 1


def _tiny_graph():
  from rigl_amd import variables as V
  g = V.Graph(DEV)
  rs = np.random.RandomState(3)
  a = g.add_masked_layer('conv_a', (3, 3, 8, 16), True, weight_decay=1e-4, init=rs.randn(3, 3, 8, 16))
  g.add_masked_layer('conv_b', (1, 1, 16, 24), True, weight_decay=5e-4, init=rs.randn(1, 1, 16, 24))
  g.add_masked_layer('fc', (24, 10), False, weight_decay=1e-4, init=rs.randn(24, 10))
  g.add_variable('bn/gamma', (24,), V.KIND_OTHER, init=rs.randn(24))
  a.mask.assign((rs.rand(3, 3, 8, 16) < 0.25).astype(np.float32))
  g.layers[1].mask.assign((rs.rand(1, 1, 16, 24) < 0.5).astype(np.float32))
  g.finalize()
  return g, rs


def _graph_reference(g, layout, grad_scale=1.0):
  """The reference of the record the next apply writes, from the arenas as they are now."""
  Wh, Gh, Bh = g.W.cpu().numpy(), g.G.cpu().numpy(), g.BITS.cpu().numpy().view(np.uint32)
  out = []
  for l, v in zip(layout, sorted(g.trainable_variables(), key=lambda v: v.offset)):
    assert l['name'] == v.name
    wd = v.weight_decay if v.kind != 2 else 0.0
    e = {'n': v.numel, 'w_buf': Wh[v.offset:], 'g_buf': Gh[v.offset:], 'bits': Bh[v.offset // 32:] if l['mask'] else None,
         'weight_decay': wd, 'apply_mask': 1}
    out.append(R.entry_sums(e, grad_scale))
  return out


def test_ring_of_4_slots_and_11_steps_through_read():
  """TrainingSummaries on a small graph and a plain gradient-descent optimizer: 11 applied steps into 4 slots leave steps 7..10
  and 7 dropped; the surviving records are those of the arenas each step saw."""
  from rigl_amd import summaries as S, train
  g, rs = _tiny_graph()
  opt = train.GradientDescentOptimizer(0.05, graph=g)
  gs = g.get_or_create_global_step()
  summ = S.TrainingSummaries(g, opt, ring=4, steps_per_epoch=4).attach()
  refs = []
  for _ in range(11):
    g.G.copy_(torch.from_numpy(rs.randn(g.G.numel()).astype(np.float32)))
    refs.append(_graph_reference(g, summ.layout))
    opt.apply_gradients(None, global_step=gs)
  records, dropped = summ.read(per_variable=True)
  assert [r['global_step'] for r in records] == [7, 8, 9, 10] and dropped == 7
  assert summ.read() == ([], 0)
  for r in records:
    ref = refs[r['global_step']]
    assert r['learning_rate'] == float(F32(0.05)) and r['current_epoch'] == r['global_step'] / 4.0
    assert math.isnan(r['cross_loss'])                                      # apply_gradients without a backpropagated loss
    assert 'drop_fraction' not in r
    n_all = sum(l['n'] for l in summ.layout)
    for k in R.FLOAT_FIELDS:
      for l, e in zip(summ.layout, ref):
        assert R.float_ok(r['per_variable'][l['name']][k], e[k], l['n'])
    for k in R.COUNT_FIELDS:
      assert [r['per_variable'][l['name']][k] for l in summ.layout] == [e[k] for e in ref]
    sg = math.fsum(e['sumsq_g'] for e in ref)
    sw = math.fsum(e['sumsq_w'] for e in ref)
    assert abs(r['grad_norm'] ** 2 - sg) <= R.bound(n_all, sg) + 4 * 2.0 ** -53 * sg   # (+ the root and its square)
    assert abs(r['var_norm'] ** 2 - sw) <= R.bound(n_all, sw) + 4 * 2.0 ** -53 * sw
    assert r['fw_nz_mask'] == ref[0]['mask_ones'] and r['fw_nz_weight'] == ref[0]['nz_w']
    assert r['pruning/conv_a/mask/sparsity'] == float(F32(1) - F32(F32(ref[0]['mask_ones']) / F32(3 * 3 * 8 * 16)))
    assert set(S.mask_summaries(g.get_masks())) == {'pruning/conv_a/mask/sparsity', 'pruning/conv_b/mask/sparsity'}
    assert r['pruning/conv_a/mask/sparsity'] == S.mask_summaries(g.get_masks())['pruning/conv_a/mask/sparsity']
  # detached: the optimizer enqueues no summary launch and the ring stays as it is
  summ.detach()
  assert opt.summary_hook is None
  opt.apply_gradients(None, global_step=gs)
  assert summ.read() == ([], 0)
