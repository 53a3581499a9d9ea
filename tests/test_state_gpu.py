"""rigl_state_gather / rigl_state_scatter against tests/state_ref.py on every case of its set, at max_blocks 0 / 1 / 3:

  * zero differing bytes against the reference image (gather) or the regions' data (scatter), the digests equal the reference's;
  * 1 MiB guards in front of and behind the packed image and around every region intact; the source side is left unchanged;
    a second run gives the same bytes;
  * the scatter is handed an image whose padding holds garbage: it never reads it;
  * through the guarded workspace at exactly the queried size, both poison fills give identical bits;
  * every bad call the header lists is refused with nothing written.
"""
import ctypes as C

import numpy as np
import pytest

from tests import state_ref as R
from tests import wsguard

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
POISON = 0xFF
FILL = 0x5C                      # what outputs hold in front of a call that must be refused


_REF = {}


def _ref(name):
  """(regions, image, digests) of a case, computed once."""
  if name not in _REF:
    regs = R.CASES[name].regions()
    _REF[name] = (regs,) + R.image(regs)
  return _REF[name]


class _Device:
  """The carved region buffer and the guarded packed buffer of a case on the device."""

  def __init__(self, name, with_data):
    case = R.CASES[name]
    regs, image, _ = _ref(name)
    total, self.spans = case.layout(R.GUARD)
    self.buf = torch.full((total,), R.SENTINEL, dtype=torch.uint8, device=DEV)
    assert self.buf.data_ptr() % 256 == 0
    if with_data:
      for (o, n), r in zip(self.spans, regs):
        if n:
          self.buf[o:o + n].copy_(torch.from_numpy(r.view(np.uint8)))
    self.views = [self.buf[o:o + n] for o, n in self.spans]
    for v, s in zip(self.views, case.shift):
      assert v.numel() == 0 or (v.data_ptr() % 16) // 4 == s
    self.nbytes = image.size
    self.pk = torch.full((2 * R.GUARD + max(self.nbytes, 256),), R.SENTINEL, dtype=torch.uint8, device=DEV)
    self.packed = self.pk[R.GUARD:R.GUARD + max(self.nbytes, 256)]
    self.packed.fill_(POISON)
    self.digests = torch.full((2 * len(regs),), -1, dtype=torch.int64, device=DEV)

  def regions_intact(self):
    """Every byte of the region buffer outside the regions is the sentinel."""
    flags, prev = [], 0
    for o, n in self.spans + [(self.buf.numel(), 0)]:
      flags.append((self.buf[prev:o] != R.SENTINEL).any())
      prev = o + n
    return not bool(torch.stack(flags).any())

  def packed_guards_intact(self):
    n = self.packed.numel()
    return not bool((self.pk[:R.GUARD] != R.SENTINEL).any() | (self.pk[R.GUARD + n:] != R.SENTINEL).any())

  def read_digests(self):
    d = self.digests.cpu().numpy().view(np.uint64)
    return [(int(d[2 * i]), int(d[2 * i + 1])) for i in range(d.size // 2)]


@pytest.mark.parametrize('max_blocks', [0, 1, 3])
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_gather(name, max_blocks):
  from rigl_amd import ops
  regs, image, digests = _ref(name)
  d = _Device(name, with_data=True)
  src0 = d.buf.clone()
  table = ops.state_table(d.views)
  assert ops.state_packed_bytes(table) == image.size
  runs = []
  for _ in range(2):
    d.packed.fill_(POISON)
    d.digests.fill_(-1)
    ops.state_gather(table, d.packed, d.digests, max_blocks=max_blocks)
    runs.append((d.packed[:d.nbytes].cpu().numpy().copy(), d.read_digests()))
  assert int(np.count_nonzero(runs[0][0] != image)) == 0
  assert runs[0][1] == digests
  assert np.array_equal(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
  assert d.packed_guards_intact() and bool((d.packed[d.nbytes:] == POISON).all())
  assert torch.equal(d.buf, src0)                           # the regions and their guards: only read


@pytest.mark.parametrize('max_blocks', [0, 1, 3])
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_scatter(name, max_blocks):
  from rigl_amd import ops
  regs, image, digests = _ref(name)
  d = _Device(name, with_data=False)
  garbage = image.copy()                                     # the padding holds garbage: the scatter must not read it
  offs, _ = R.offsets([4 * r.size for r in regs])
  for r, o in zip(regs, offs):
    garbage[o + 4 * r.size:o + R.pad(4 * r.size)] = 0xEE
  if d.nbytes:
    d.packed[:d.nbytes].copy_(torch.from_numpy(garbage))
  pk0 = d.pk.clone()
  table = ops.state_table(d.views)
  runs = []
  for _ in range(2):
    for v in d.views:
      v.fill_(R.SENTINEL)
    d.digests.fill_(-1)
    ops.state_scatter(table, d.packed, d.digests, max_blocks=max_blocks)
    runs.append(([v.cpu().numpy().copy() for v in d.views], d.read_digests()))
  for got, r in zip(runs[0][0], regs):
    assert int(np.count_nonzero(got != r.view(np.uint8))) == 0
  assert runs[0][1] == digests and runs[1][1] == digests
  assert all(np.array_equal(a, b) for a, b in zip(runs[0][0], runs[1][0]))
  assert d.regions_intact()
  assert torch.equal(d.pk, pk0)                              # the image and its guards: only read


@pytest.mark.parametrize('name', ['edges', 'table_129'])
def test_through_the_workspace_guard_at_exactly_the_queried_size(name):
  from rigl_amd import ops
  regs, image, digests = _ref(name)
  outs = []
  for poison in wsguard.POISONS:
    g = wsguard.GuardedWorkspace(poison=poison)
    with wsguard.installed(g):
      d = _Device(name, with_data=True)
      table = ops.state_table(d.views)
      need = ops.state_workspace_bytes(table)
      ops.state_gather(table, d.packed, d.digests)
      log = g.check('gather')
      assert [(t, n) for t, n, _ in log] == [('state', need)]
      gathered = (d.packed[:d.nbytes].cpu().numpy().copy(), d.read_digests())
      for v in d.views:
        v.fill_(R.SENTINEL)
      d.digests.fill_(-1)
      ops.state_scatter(table, d.packed, d.digests)
      log = g.check('scatter')
      assert [(t, n) for t, n, _ in log] == [('state', need)]
      outs.append(gathered + ([v.cpu().numpy().copy() for v in d.views], d.read_digests()))
      assert d.regions_intact() and d.packed_guards_intact()
  a, b = outs
  assert np.array_equal(a[0], b[0]) and a[1] == b[1] == digests and a[3] == b[3] == digests
  assert np.array_equal(a[0], image)
  assert all(np.array_equal(x, y) and np.array_equal(x, r.view(np.uint8)) for x, y, r in zip(a[2], b[2], regs))


def _bad_calls():
  """(what, expected code name, a function (regions pointer values, bufs) -> call arguments)."""
  ok = dict(shift=0, bytes=None, null=False, packed=0, digests=0, n=None, max_blocks=0, ws='ok')
  out = []
  for what, code, kw in [
      ('a region pointer off 4-byte alignment', 'RIGL_EINVAL', dict(shift=2)),
      ('negative bytes', 'RIGL_EINVAL', dict(bytes=-4)),
      ('bytes no multiple of 4', 'RIGL_EINVAL', dict(bytes=6)),
      ('a NULL pointer with bytes > 0', 'RIGL_EINVAL', dict(null=True)),
      ('packed off 256-byte alignment', 'RIGL_EINVAL', dict(packed=128)),
      ('digests off 8-byte alignment', 'RIGL_EINVAL', dict(digests=4)),
      ('n < 0', 'RIGL_EINVAL', dict(n=-1)),
      ('max_blocks < 0', 'RIGL_EINVAL', dict(max_blocks=-1)),
      ('a NULL workspace', 'RIGL_EWORKSPACE', dict(ws='null')),
      ('a workspace of need - 1 bytes', 'RIGL_EWORKSPACE', dict(ws='short'))]:
    out.append((what, code, dict(ok, **kw)))
  return out


@pytest.mark.parametrize('fn', ['rigl_state_gather', 'rigl_state_scatter'])
def test_bad_calls_are_refused_with_nothing_written(fn):
  from rigl_amd import _lib
  lib = _lib.load()
  words = [100, 0, 5000]
  bufs = [torch.full((4 * w + 16,), FILL, dtype=torch.uint8, device=DEV) for w in words]
  packed = torch.full((R.offsets([4 * w for w in words])[1] + 256,), FILL, dtype=torch.uint8, device=DEV)
  digests = torch.full((8,), FILL, dtype=torch.uint8, device=DEV).repeat(len(words) * 2 + 1)
  good = (_lib.StateRegion * 3)(*[_lib.StateRegion(b.data_ptr(), 4 * w) for b, w in zip(bufs, words)])
  need = lib.rigl_state_workspace_bytes(good, 3)
  assert need > 0 and lib.rigl_state_packed_bytes(good, 3) == packed.numel() - 256
  ws = torch.full((need,), FILL, dtype=torch.uint8, device=DEV)
  stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
  for what, code, k in _bad_calls():
    arr = (_lib.StateRegion * 3)(*[_lib.StateRegion(b.data_ptr(), 4 * w) for b, w in zip(bufs, words)])
    arr[2].ptr = None if k['null'] else bufs[2].data_ptr() + k['shift']
    if k['bytes'] is not None:
      arr[2].bytes = k['bytes']
    wsp, wsn = {'ok': (ws.data_ptr(), need), 'null': (None, need), 'short': (ws.data_ptr(), need - 1)}[k['ws']]
    rc = getattr(lib, fn)(arr, 3 if k['n'] is None else k['n'], packed.data_ptr() + k['packed'], digests.data_ptr() + k['digests'],
                          wsp, wsn, k['max_blocks'], stream)
    assert rc == getattr(_lib, code), '%s with %s: returned %d (%s), not %s' % (
        fn, what, rc, lib.rigl_last_error().decode('utf-8', 'replace'), code)
    assert fn.encode() in lib.rigl_last_error()
  torch.cuda.synchronize()
  for t in bufs + [packed, digests, ws]:
    assert bool((t == FILL).all()), fn + ': a refused call wrote something'
  # the queries answer 0 for a malformed table; a table without regions is legal and launches nothing
  bad = (_lib.StateRegion * 1)(_lib.StateRegion(bufs[0].data_ptr(), 6))
  assert lib.rigl_state_packed_bytes(bad, 1) == 0 and lib.rigl_state_workspace_bytes(bad, 1) == 0
  assert getattr(lib, fn)(None, 0, None, None, None, 0, 0, stream) == _lib.RIGL_OK
