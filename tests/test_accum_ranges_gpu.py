"""rigl_grad_accumulate_ranges on the GPU against tests/accum_ranges_ref.py: every case x mode x grid cap (1, 3 and the default)
leaves zero differing bits (NaN positions compared as NaN-ness where the mode adds); guards, gaps, slack and the arena a mode does
not write are bit-identical to their poison; the FIRST / ADD / LAST chain ends where the reference's does; one range covering the
arena gives the bits of rigl_grad_accumulate, and so does any way of cutting the same elements into ranges; every bad call is
refused with RIGL_EINVAL and nothing written."""
import ctypes as C

import numpy as np
import pytest

import accum_ranges_ref as R

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = R.build_cases()
IDS = [c['name'] for c in CASES]
BY_NAME = {c['name']: c for c in CASES}


def _table(ranges):
  from rigl_amd import _lib
  arr = (_lib.AccRange * max(len(ranges), 1))()
  for i, (off, ln) in enumerate(ranges):
    arr[i].offset, arr[i].length = off, ln
  return arr


def _call(t, lay, ranges, mode, inv_k, max_blocks, n=None, n_ranges=None, table=True, ptrs=None, acc_off=None, g_off=None):
  """The C entry point on the words of device tensor ``t`` (int32); returns its status."""
  from rigl_amd import _lib, ops
  base = t.data_ptr()
  at = lambda off: C.c_void_p(base + 4 * off)
  p = dict(acc=at(lay['acc'] if acc_off is None else acc_off), g=at(lay['g'] if g_off is None else g_off), loss=at(lay['loss']),
           loss_acc=at(lay['loss_acc']), loss_mean=at(lay['loss_mean']))
  p.update(ptrs or {})
  return _lib.load().rigl_grad_accumulate_ranges(
      lay['n'] if n is None else n, p['acc'], p['g'], _table(ranges) if table else None,
      len(ranges) if n_ranges is None else n_ranges, int(mode), p['loss'], p['loss_acc'], p['loss_mean'], float(inv_k),
      int(max_blocks), ops._stream())


def _kernel(buf, lay, ranges, mode, inv_k, max_blocks):
  from rigl_amd import _lib
  t = torch.from_numpy(buf.view(np.int32)).to(DEV)
  assert t.data_ptr() % 256 == 0
  assert _call(t, lay, ranges, mode, inv_k, max_blocks) == _lib.RIGL_OK
  buf[:] = t.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('max_blocks', R.MAX_BLOCKS)
@pytest.mark.parametrize('mode', R.MODES, ids=['first', 'add', 'last'])
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_stage_matches_the_reference(case, mode, max_blocks):
  assert R.check_stage(_kernel, case, mode, max_blocks) == []


@pytest.mark.parametrize('max_blocks', R.MAX_BLOCKS)
@pytest.mark.parametrize('case', CASES, ids=IDS)
def test_chain_matches_the_reference(case, max_blocks):
  assert R.check_chain(_kernel, case, max_blocks) == []


@pytest.mark.parametrize('mode', R.MODES, ids=['first', 'add', 'last'])
def test_one_range_over_the_arena_gives_the_bits_of_the_whole_arena_pass(mode):
  from rigl_amd import _lib, ops
  case = BY_NAME['whole_arena']
  assert case['ranges'] == [(0, case['n'])]
  before, lay = R.state_before(case, mode)
  a = torch.from_numpy(before.view(np.int32)).to(DEV)
  b = a.clone()
  assert _call(a, lay, case['ranges'], mode, R.INV_K, 0) == _lib.RIGL_OK
  at = lambda k: C.c_void_p(b.data_ptr() + 4 * lay[k])
  assert _lib.load().rigl_grad_accumulate(lay['n'], at('acc'), at('g'), int(mode), at('loss'), at('loss_acc'), at('loss_mean'),
                                          float(R.INV_K), 0, ops._stream()) == _lib.RIGL_OK
  assert torch.equal(a, b)
  assert not torch.equal(a.cpu(), torch.from_numpy(before.view(np.int32)))


@pytest.mark.parametrize('mode', R.MODES, ids=['first', 'add', 'last'])
def test_the_bits_do_not_depend_on_how_the_elements_are_cut_into_ranges(mode):
  from rigl_amd import _lib
  case = BY_NAME['whole_arena']
  n = case['n']
  before, lay = R.state_before(case, mode)
  want = before.copy()
  _kernel(want, lay, case['ranges'], mode, R.INV_K, 0)
  cuts = [0, 4, 8, 4096, 4100, 8192, 8192, 8448, n]                   # eight touching ranges, one of them empty
  got = before.copy()
  _kernel(got, lay, [(lo, hi - lo) for lo, hi in zip(cuts, cuts[1:])], mode, R.INV_K, 3)
  np.testing.assert_array_equal(got, want)
  # ... and two launches, each with half of the elements and one of them with the loss, are one launch
  t = torch.from_numpy(before.view(np.int32)).to(DEV)
  null = C.c_void_p(0)
  assert _call(t, lay, [(0, 4100)], mode, R.INV_K, 0, ptrs=dict(loss=null)) == _lib.RIGL_OK
  assert _call(t, lay, [(4100, n - 4100)], mode, R.INV_K, 1) == _lib.RIGL_OK
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want)


@pytest.mark.parametrize('mode', R.MODES, ids=['first', 'add', 'last'])
def test_without_a_loss_no_scalar_is_touched(mode):
  case = BY_NAME['head_and_tail']
  before, lay = R.state_before(case, mode)
  want = before.copy()
  R.reference(want, lay, case['ranges'], mode, R.INV_K)
  for k in ('loss_acc', 'loss_mean'):
    want[lay[k]] = before[lay[k]]
  t = torch.from_numpy(before.view(np.int32)).to(DEV)
  null = C.c_void_p(0)
  assert _call(t, lay, case['ranges'], mode, R.INV_K, 0, ptrs=dict(loss=null, loss_acc=null, loss_mean=null)) == 0
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want)
  # an empty table without a loss: nothing to do
  assert _call(t, lay, [], mode, R.INV_K, 0, ptrs=dict(loss=null, loss_acc=null, loss_mean=null)) == 0
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), want)


def test_bad_calls_are_refused_and_write_nothing():
  from rigl_amd import _lib
  case = BY_NAME['two_gap4']
  before, lay = R.state_before(case, R.ADD)
  n = lay['n']
  t = torch.from_numpy(before.view(np.int32)).to(DEV)
  null = C.c_void_p(0)
  ok = case['ranges']
  bad = [
      dict(ranges=[(4 * i, 4) for i in range(9)]),                                  # more than 8 ranges
      dict(n_ranges=9), dict(n_ranges=-1), dict(table=False),                       # ... by count; a NULL table
      dict(ranges=[(n // 4 * 4 - 4, 8)]), dict(ranges=[(0, n + 1)]), dict(ranges=[(n // 4 * 4 + 4, 0)]),   # past n
      dict(ranges=[(0, 8), (8, 2 ** 62)]), dict(ranges=[(2 ** 62, 4)]),                            # ... far past n
      dict(ranges=[(0, 9), (8, 4)]), dict(ranges=[(0, 8), (4, 8)]), dict(ranges=[(0, 64), (0, 64)]),   # overlapping
      dict(ranges=[(64, 8), (0, 8)]), dict(ranges=[(8, 0), (4, 0)]),                               # not ascending
      dict(ranges=[(2, 8)]), dict(ranges=[(0, 4), (5, 4)]), dict(ranges=[(7, 0)]),                 # offset % 4
      dict(ranges=[(-4, 8)]), dict(ranges=[(0, -1)]),                                              # negative
      # everything rigl_grad_accumulate refuses
      dict(acc_off=lay['acc'] + 1), dict(g_off=lay['g'] + 2), dict(acc_off=lay['acc'] + 3, g_off=lay['g'] + 3),
      dict(ptrs=dict(acc=null)), dict(ptrs=dict(g=null)), dict(g_off=lay['acc']),
      dict(mode=3), dict(mode=-1), dict(n=-1), dict(max_blocks=-1),
      dict(ptrs=dict(loss_acc=null)), dict(mode=R.LAST, ptrs=dict(loss_mean=null)),
      dict(ptrs=dict(loss=C.c_void_p(t.data_ptr() + 4 * lay['loss'] + 2))),
  ]
  for kw in bad:
    kw = dict(kw)
    mode, mb, ranges = kw.pop('mode', R.ADD), kw.pop('max_blocks', 0), kw.pop('ranges', ok)
    assert _call(t, lay, ranges, mode, R.INV_K, mb, **kw) == _lib.RIGL_EINVAL, kw
    assert b'rigl_grad_accumulate_ranges' in _lib.load().rigl_last_error()
  torch.cuda.synchronize()
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), before)
  assert _call(t, lay, ok, R.ADD, R.INV_K, 0) == _lib.RIGL_OK                       # the call the bad ones were derived from


def test_ops_wrapper_checks_and_accumulates():
  from rigl_amd import _lib, ops
  n = 3 * R.TILE + 5
  rng = np.random.default_rng(7)
  g1, g2 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
  acc = torch.from_numpy(g1).to(DEV)
  g = torch.from_numpy(g2).to(DEV)
  l, la, lm = torch.tensor([2.25], device=DEV), torch.tensor([1.5], device=DEV), torch.zeros(1, device=DEV)
  ranges = [(64, R.TILE + 3), (2 * R.TILE, R.TILE + 5)]
  ops.grad_accumulate_ranges(acc, g, ranges, _lib.ACC_LAST, loss=l, loss_acc=la, loss_mean=lm, inv_k=0.5)
  want = g2.copy()
  for off, ln in ranges:
    want[off:off + ln] = g1[off:off + ln] + g2[off:off + ln]
  np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), want.view(np.uint32))
  np.testing.assert_array_equal(acc.cpu().numpy().view(np.uint32), g1.view(np.uint32))
  assert float(lm) == (1.5 + 2.25) * 0.5 and float(la) == 1.5
  ops.grad_accumulate_ranges(acc, g, [], _lib.ACC_ADD, loss=l, loss_acc=la)          # no range: the loss arithmetic alone
  assert float(la) == 3.75
  np.testing.assert_array_equal(acc.cpu().numpy().view(np.uint32), g1.view(np.uint32))
  with pytest.raises(ValueError):
    ops.grad_accumulate_ranges(acc[:-1], g, ranges, _lib.ACC_ADD)
  with pytest.raises(TypeError):
    ops.grad_accumulate_ranges(acc.double(), g, ranges, _lib.ACC_ADD)
  with pytest.raises(_lib.RiglError):
    ops.grad_accumulate_ranges(acc.cpu(), g, ranges, _lib.ACC_ADD)
  with pytest.raises(_lib.RiglError):
    ops.grad_accumulate_ranges(acc, g, [(0, 8), (4, 8)], _lib.ACC_ADD)
  with pytest.raises(_lib.RiglError):
    ops.grad_accumulate_ranges(acc, g, [(0, 4)] * 9, _lib.ACC_ADD)
