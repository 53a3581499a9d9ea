"""rigl_grad_accumulate on the GPU against tests/accum_ref.py: every case x mode x max_blocks leaves zero differing bits (NaN
positions compared as NaN-ness where the mode adds), guards, slack and the operands a mode does not write intact, and the same
bits on a second run; the FIRST / ADD / LAST chain ends where the reference's does; bad calls are refused with nothing written."""
import ctypes as C

import numpy as np
import pytest

import accum_ref as R

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = R.build_cases()
IDS = [c['name'] for c in CASES]


def _call(t, lay, mode, inv_k, max_blocks, acc_off=None, g_off=None, loss=True, n=None, ptrs=None):
  """The C entry point on the words of device tensor ``t`` (int32); returns its status."""
  from rigl_amd import _lib, ops
  base = t.data_ptr()
  at = lambda off: C.c_void_p(base + 4 * off) if off is not None else C.c_void_p(0)
  p = dict(acc=at(lay['acc'] if acc_off is None else acc_off), g=at(lay['g'] if g_off is None else g_off),
           loss=at(lay['loss'] if loss else None), loss_acc=at(lay['loss_acc']), loss_mean=at(lay['loss_mean']))
  p.update(ptrs or {})
  return _lib.load().rigl_grad_accumulate(lay['n'] if n is None else n, p['acc'], p['g'], int(mode), p['loss'], p['loss_acc'],
                                          p['loss_mean'], float(inv_k), int(max_blocks), ops._stream())


def _kernel(buf, lay, mode, inv_k, max_blocks):
  from rigl_amd import _lib
  t = torch.from_numpy(buf.view(np.int32)).to(DEV)
  assert t.data_ptr() % 256 == 0
  assert _call(t, lay, mode, inv_k, max_blocks) == _lib.RIGL_OK
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
def test_without_a_loss_no_scalar_is_touched(mode):
  case = next(c for c in CASES if c['name'] == 'size_%d' % (R.TILE + 1))
  before, lay = R.state_before(case, mode)
  want = before.copy()
  R.reference(want, lay, mode, 1.0 / 3)
  for k in ('loss_acc', 'loss_mean'):
    want[lay[k]] = before[lay[k]]
  t = torch.from_numpy(before.view(np.int32)).to(DEV)
  assert _call(t, lay, mode, 1.0 / 3, 0, loss=False, ptrs=dict(loss_acc=C.c_void_p(0), loss_mean=C.c_void_p(0))) == 0
  got = t.cpu().numpy().view(np.uint32)
  assert R.compare(got, want, lay, [mode]) == []


def test_bad_calls_are_refused_and_write_nothing():
  from rigl_amd import _lib
  case = next(c for c in CASES if c['name'] == 'size_%d' % (R.WAVE + 1))
  before, lay = R.state_before(case, R.ADD)
  t = torch.from_numpy(before.view(np.int32)).to(DEV)
  null = C.c_void_p(0)
  bad = [
      dict(acc_off=lay['acc'] + 1), dict(g_off=lay['g'] + 2), dict(acc_off=lay['acc'] + 3, g_off=lay['g'] + 3),   # misaligned
      dict(ptrs=dict(acc=null)), dict(ptrs=dict(g=null)), dict(g_off=lay['acc']),                                 # NULL, acc == grad
      dict(mode=3), dict(mode=-1), dict(n=-1), dict(max_blocks=-1),
      dict(ptrs=dict(loss_acc=null)), dict(mode=R.LAST, ptrs=dict(loss_mean=null)),
  ]
  for kw in bad:
    kw = dict(kw)
    mode, mb = kw.pop('mode', R.ADD), kw.pop('max_blocks', 0)
    assert _call(t, lay, mode, 1.0 / 3, mb, **kw) == _lib.RIGL_EINVAL, kw
  torch.cuda.synchronize()
  np.testing.assert_array_equal(t.cpu().numpy().view(np.uint32), before)


def test_ops_wrapper_checks_and_accumulates():
  from rigl_amd import _lib, ops
  n = 2 * R.TILE + 5
  rng = np.random.default_rng(7)
  g1, g2 = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
  acc = torch.full((n,), float('nan'), device=DEV)
  g = torch.from_numpy(g1).to(DEV)
  l, la, lm = torch.tensor([1.5], device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
  ops.grad_accumulate(acc, g, _lib.ACC_FIRST, loss=l, loss_acc=la)
  g.copy_(torch.from_numpy(g2))
  l.fill_(2.25)
  ops.grad_accumulate(acc, g, _lib.ACC_LAST, loss=l, loss_acc=la, loss_mean=lm, inv_k=0.5)
  np.testing.assert_array_equal(g.cpu().numpy().view(np.uint32), (g1 + g2).view(np.uint32))
  np.testing.assert_array_equal(acc.cpu().numpy().view(np.uint32), g1.view(np.uint32))
  assert float(lm) == (1.5 + 2.25) * 0.5 and float(la) == 1.5
  with pytest.raises(ValueError):
    ops.grad_accumulate(acc[:-1], g, _lib.ACC_ADD)
  with pytest.raises(TypeError):
    ops.grad_accumulate(acc.double(), g, _lib.ACC_ADD)
  with pytest.raises(_lib.RiglError):
    ops.grad_accumulate(acc.cpu(), g, _lib.ACC_ADD)
  with pytest.raises(_lib.RiglError):
    ops.grad_accumulate(acc, g, 7)
