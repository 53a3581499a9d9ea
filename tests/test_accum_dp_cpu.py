"""The host protocol between train.MicroBatches and dist.GradSync, on a CPU graph with a gloo group of one rank (no device
compute): a held exchange enqueues nothing and keeps no bucket state; ``before_exchange`` sees every arena element exactly once,
each range in front of its own collective and the flush's two ranges in one call; a GradSync over another graph is refused; a
snapshot is refused while an exchange is held or armed; rigl_grad_accumulate_ranges refuses bad tables before touching a device."""
import ctypes as C
import os
import socket

import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


@pytest.fixture()
def one_rank(monkeypatch):
  """A gloo group of one rank, torch.distributed.all_reduce wrapped to log what it is given."""
  monkeypatch.syspath_prepend(ROOT)
  monkeypatch.setenv('MASTER_ADDR', '127.0.0.1')
  monkeypatch.setenv('MASTER_PORT', str(_free_port()))
  import torch.distributed as dist
  dist.init_process_group('gloo', rank=0, world_size=1)
  log = []
  real = dist.all_reduce

  def all_reduce(t, *a, **kw):
    log.append(('all_reduce', t.data_ptr(), t.numel()))
    return real(t, *a, **kw)
  monkeypatch.setattr(dist, 'all_reduce', all_reduce)
  try:
    yield log
  finally:
    dist.destroy_process_group()


def _graph():
  from rigl_amd import variables as V
  g = V.Graph('cpu')
  vs = [g.add_variable('l%d/weights' % i, (3, 3, 16, 16), V.KIND_MASKED) for i in range(6)]
  bn = g.add_variable('bn/gamma', (64,), V.KIND_OTHER)
  g.finalize()
  return g, vs, bn


def _backward(sync, vs, bn, value):
  for v in sorted(vs, key=lambda v: -v.offset):
    v.grad.fill_(value)
    sync.notify_layer_grad_ready(v)
  bn.grad.fill_(2 * value)
  sync.all_reduce(sync.graph)


def test_a_held_exchange_enqueues_nothing_and_keeps_no_bucket_state(one_rank):
  from rigl_amd.dist import GradSync
  g, vs, bn = _graph()
  s = GradSync(g, bucket_bytes=4 * 3000, enabled=True)
  assert s.held is False and s.before_exchange is None
  s.held = True
  _backward(s, vs, bn, 1.0)
  assert one_rank == [] and s._hi is None and s._handles == [] and s._timeline == [] and not s._ready     # pylint: disable=protected-access
  s.held = False
  _backward(s, vs, bn, 3.0)                                  # the next pass is a whole exchange, as if the held one never ran
  assert len(one_rank) == s.n_buckets_last >= 3
  assert sum(n for _, _, n in one_rank) == g.G.numel()
  assert sum(r['bytes'] for r in s.timeline_summary()['buckets']) == 4 * g.G.numel()


def test_before_exchange_sees_every_element_once_in_front_of_its_collective(one_rank):
  from rigl_amd import variables as V
  from rigl_amd.dist import GradSync
  g, vs, bn = _graph()
  s = GradSync(g, bucket_bytes=4 * 3000, enabled=True)
  base, kend, end = g.G.data_ptr(), g.seg[V.KIND_DENSE][1], g.G.numel()
  s.before_exchange = lambda ranges, final: one_rank.append(('before', list(ranges), final))
  _backward(s, vs, bn, 1.0)
  hooks = [e for e in one_rank if e[0] == 'before']
  assert [e[2] for e in hooks] == [False] * (len(hooks) - 1) + [True] and len(hooks) >= 3
  assert all(len(e[1]) == 1 for e in hooks[:-1])
  assert hooks[-1][1][-1] == (kend, end)                      # the flush: what is left of the kernel segment, and BN / bias
  seen = torch.zeros(end, dtype=torch.int32)
  for e in hooks:
    for lo, hi in e[1]:
      assert lo % 4 == 0 and hi > lo
      seen[lo:hi] += 1
  assert torch.all(seen == 1)
  # every range is announced BEFORE the collective that sends it, and nothing else is sent
  announced = set()
  for e in one_rank:
    if e[0] == 'before':
      announced |= {(base + 4 * lo, hi - lo) for lo, hi in e[1]}
    else:
      assert (e[1], e[2]) in announced
      announced.discard((e[1], e[2]))
  assert not announced
  # a model that notifies no layer: everything is the flush's
  del one_rank[:]
  bn.grad.fill_(1.0)
  s.all_reduce(g)
  assert one_rank[0] == ('before', [(0, kend), (kend, end)], True) and len(one_rank) == 3


def test_micro_batches_refuses_an_exchange_over_another_graph(one_rank):
  from rigl_amd import train
  from rigl_amd.dist import GradSync
  g, _, _ = _graph()
  other, _, _ = _graph()
  inner = train.GradientDescentOptimizer(0.1, graph=g, grad_sync=GradSync(other, enabled=True))
  with pytest.raises(NotImplementedError, match='graph'):
    train.MicroBatches(lambda: None, inner, 1)
  inner = train.GradientDescentOptimizer(0.1, graph=g, grad_sync=GradSync(g, enabled=True))
  mb = train.MicroBatches(lambda: None, inner, 1)            # the optimizer's own graph, forced on with one rank: accepted
  assert mb._sync is inner._grad_sync and mb._arena is None  # pylint: disable=protected-access
  inner = train.GradientDescentOptimizer(0.1, graph=g, grad_sync=GradSync(other, enabled=False))
  assert train.MicroBatches(lambda: None, inner, 1)._sync is None   # pylint: disable=protected-access


def test_a_snapshot_is_refused_while_the_exchange_is_held_or_armed(one_rank):
  from rigl_amd import checkpoint, train
  from rigl_amd.dist import GradSync
  g, _, _ = _graph()
  sync = GradSync(g, enabled=True)
  inner = train.MomentumOptimizer(0.1, 0.9, graph=g, grad_sync=sync)
  state = checkpoint.TrainingState(g, inner)
  state.snapshot()
  sync.held = True
  with pytest.raises(RuntimeError, match='pending'):
    state.snapshot()
  sync.held = False
  sync.before_exchange = lambda ranges, final: None
  with pytest.raises(RuntimeError, match='pending'):
    state.snapshot()
  with pytest.raises(RuntimeError, match='pending'):
    state.restore('nowhere')
  sync.before_exchange = None
  state.snapshot()


def test_the_ranges_entry_point_refuses_bad_tables_without_a_device():
  """(On a thread of its own: the library's error message is per thread, and the main thread's stays as it was.)"""
  import threading
  failed = []

  def run():
    try:
      _refusals()
    except BaseException as e:  # pylint: disable=broad-except
      failed.append(e)
  t = threading.Thread(target=run)
  t.start()
  t.join()
  if failed:
    raise failed[0]


def _refusals():
  from rigl_amd import _lib
  lib = _lib.load()
  fake = lambda a: C.c_void_p(a)                             # never dereferenced: every call below is refused first

  def call(ranges, n=1000, mode=_lib.ACC_ADD, n_ranges=None, acc=4096, grad=1 << 20, table=True, max_blocks=0):
    arr = (_lib.AccRange * max(len(ranges), 1))()
    for i, (off, ln) in enumerate(ranges):
      arr[i].offset, arr[i].length = off, ln
    return lib.rigl_grad_accumulate_ranges(n, fake(acc), fake(grad), arr if table else None,
                                           len(ranges) if n_ranges is None else n_ranges, mode, None, None, None, 1.0, max_blocks,
                                           None)
  bad = [dict(ranges=[(4 * i, 4) for i in range(9)]), dict(ranges=[], n_ranges=9), dict(ranges=[], n_ranges=-1),
         dict(ranges=[(0, 4)], table=False), dict(ranges=[(996, 8)]), dict(ranges=[(0, 1001)]), dict(ranges=[(1004, 0)]),
         dict(ranges=[(2 ** 62, 4)]), dict(ranges=[(0, 8), (8, 2 ** 62)]), dict(ranges=[(0, 9), (8, 4)]),
         dict(ranges=[(0, 8), (4, 8)]), dict(ranges=[(64, 8), (0, 8)]), dict(ranges=[(8, 0), (4, 0)]), dict(ranges=[(2, 8)]),
         dict(ranges=[(7, 0)]), dict(ranges=[(-4, 8)]), dict(ranges=[(0, -1)]), dict(ranges=[(0, 4)], n=-1),
         dict(ranges=[(0, 4)], mode=3), dict(ranges=[(0, 4)], max_blocks=-1), dict(ranges=[(0, 4)], acc=4100),
         dict(ranges=[(0, 4)], grad=4096), dict(ranges=[(0, 4)], acc=0)]
  for kw in bad:
    assert call(**kw) == _lib.RIGL_EINVAL, kw
    assert b'rigl_grad_accumulate_ranges' in lib.rigl_last_error()
  # legal and empty: nothing to launch (no loss, no elements)
  assert call([]) == _lib.RIGL_OK and call([(0, 0), (0, 0), (996, 0)]) == _lib.RIGL_OK
