"""rigl_masked_sgd_momentum_dlr / rigl_masked_adam_dlr (the learning rate read from device memory) against the by-value
entry points on the same inputs: the same kernel bodies, so the same bits in every output, and nothing past them."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 64                                  # elements after every output, pre-filled and checked
SIZES = [1, 3, 4, 63, 64, 65, 4099]         # below a quad, the n % 4 tails, one wave +- 1, more than one block with a tail
RATES = [0.0, 0.1, 1e-40, 3e38]             # 1e-40 is subnormal in fp32; 3e38 overflows most products


def _inputs(n, seed):
  rs = np.random.RandomState(seed)
  t = lambda a: torch.from_numpy(a).to(DEV)
  f = lambda: t(np.concatenate([rs.randn(n), np.full(GUARD, 777.0)]).astype(np.float32))
  words = (n + 31) // 32
  return dict(w=f(), g=f(), a=f(), v=t(np.concatenate([rs.rand(n), np.full(GUARD, 777.0)]).astype(np.float32)),
              bits=t(rs.randint(-2 ** 31, 2 ** 31, size=words, dtype=np.int64).astype(np.int32)),
              shadow=torch.full((n + GUARD,), 3.0, dtype=torch.bfloat16, device=DEV))


def _clone(d):
  return {k: v.clone() for k, v in d.items()}


def _same_bits(a, b, what):
  for k in ('w', 'a', 'v', 'shadow'):
    x, y = a[k].cpu(), b[k].cpu()
    if k == 'shadow':
      x, y = x.view(torch.int16), y.view(torch.int16)
    else:
      x, y = x.view(torch.int32), y.view(torch.int32)
    assert torch.equal(x, y), (what, k)


def _guards_intact(d, n, what):
  for k in ('w', 'a', 'v'):
    assert torch.equal(d[k][n:].cpu(), torch.full((GUARD,), 777.0)), (what, k)
  assert torch.equal(d['shadow'][n:].float().cpu(), torch.full((GUARD,), 3.0)), (what, 'shadow')


@pytest.mark.parametrize('n', SIZES)
def test_sgd_device_lr_leaves_the_bits_of_the_by_value_entry_point(n):
  from rigl_amd import ops
  base = _inputs(n, n)
  for rate in RATES:
    lr_dev = torch.tensor([rate], dtype=torch.float32).to(DEV)
    assert float(lr_dev.cpu()[0]) == float(np.float32(rate))                     # (the subnormal survives the upload)
    for sel in range(8):
      has_mom, has_mask, has_shadow = bool(sel & 4), bool(sel & 2), bool(sel & 1)
      for nesterov in ((False, True) if has_mom else (False,)):
        what = (n, rate, has_mom, has_mask, has_shadow, nesterov)
        outs = []
        for device_path in (False, True):
          d = _clone(base)
          ops.masked_sgd_momentum(
              d['w'][:n], d['g'][:n], None if device_path else rate, lr_device=lr_dev if device_path else None,
              momentum=d['a'][:n] if has_mom else None, mask_bits=d['bits'] if has_mask else None, mu=0.9,
              weight_decay=5e-4, grad_scale=0.5, nesterov=nesterov, w_shadow=d['shadow'][:n] if has_shadow else None)
          outs.append(d)
        torch.cuda.synchronize()
        _same_bits(outs[0], outs[1], what)
        _guards_intact(outs[1], n, what)
        if rate == 0.1:
          assert not torch.equal(outs[1]['w'][:n], base['w'][:n]), what          # (the update did happen)
    assert float(lr_dev.cpu()[0]) == float(np.float32(rate))                     # the kernels only read the rate


@pytest.mark.parametrize('n', SIZES)
def test_adam_device_lr_leaves_the_bits_of_the_by_value_entry_point(n):
  from rigl_amd import ops
  base = _inputs(n, 100 + n)
  bp = torch.tensor([0.9 ** 3, 0.999 ** 3], dtype=torch.float32).to(DEV)
  for rate in RATES:
    lr_dev = torch.tensor([rate], dtype=torch.float32).to(DEV)
    for sel in range(4):
      has_mask, has_shadow = bool(sel & 2), bool(sel & 1)
      what = (n, rate, has_mask, has_shadow)
      outs = []
      for device_path in (False, True):
        d = _clone(base)
        ops.masked_adam(d['w'][:n], d['g'][:n], d['a'][:n], d['v'][:n], bp, None if device_path else rate,
                        lr_device=lr_dev if device_path else None, mask_bits=d['bits'] if has_mask else None,
                        weight_decay=5e-4, grad_scale=0.5, w_shadow=d['shadow'][:n] if has_shadow else None)
        outs.append(d)
      torch.cuda.synchronize()
      _same_bits(outs[0], outs[1], what)
      _guards_intact(outs[1], n, what)
      if rate == 0.1:
        assert not torch.equal(outs[1]['w'][:n], base['w'][:n]), what


def test_a_null_or_misaligned_rate_is_refused():
  from rigl_amd import _lib, ops
  lib = _lib.load()
  n = 64
  d = _inputs(n, 7)
  before = _clone(d)
  bp = torch.tensor([0.9, 0.999], dtype=torch.float32).to(DEV)
  lr = torch.tensor([0.1, 0.1], dtype=torch.float32).to(DEV)
  p = lambda t: t.data_ptr()
  for bad in (None, p(lr) + 2, p(lr) + 1):
    assert lib.rigl_masked_sgd_momentum_dlr(n, p(d['w']), p(d['a']), p(d['g']), None, bad, 0.9, 0.0, 1.0, 1, None,
                                            None) == _lib.RIGL_EINVAL
    assert b'rigl_masked_sgd_momentum_dlr' in lib.rigl_last_error()
    assert lib.rigl_masked_adam_dlr(n, p(d['w']), p(d['a']), p(d['v']), p(d['g']), None, p(bp), bad, 0.9, 0.999, 1e-8, 0.0,
                                    1.0, None, None) == _lib.RIGL_EINVAL
    assert b'rigl_masked_adam_dlr' in lib.rigl_last_error()
  # the rules of the by-value entry points hold too: a misaligned w
  assert lib.rigl_masked_sgd_momentum_dlr(n, p(d['w']) + 4, None, p(d['g']), None, p(lr), 0.9, 0.0, 1.0, 0, None,
                                          None) == _lib.RIGL_EINVAL
  assert lib.rigl_masked_adam_dlr(n, p(d['w']), p(d['a']), None, p(d['g']), None, p(bp), p(lr), 0.9, 0.999, 1e-8, 0.0, 1.0,
                                  None, None) == _lib.RIGL_EINVAL
  torch.cuda.synchronize()
  _same_bits(before, d, 'refused calls')
  # the tensor-level wrappers: exactly one of lr / lr_device, an fp32 [1] GPU tensor
  w, g = d['w'][:n], d['g'][:n]
  with pytest.raises(ValueError, match='exactly one'):
    ops.masked_sgd_momentum(w, g, 0.1, lr_device=lr[:1])
  with pytest.raises(ValueError, match='exactly one'):
    ops.masked_sgd_momentum(w, g)
  with pytest.raises(ValueError, match='1 float'):
    ops.masked_sgd_momentum(w, g, lr_device=lr)
  with pytest.raises(TypeError):
    ops.masked_adam(w, g, d['a'][:n], d['v'][:n], bp, lr_device=lr[:1].double())
  with pytest.raises(Exception, match='GPU'):
    ops.masked_sgd_momentum(w, g, lr_device=lr[:1].cpu())
  _same_bits(before, d, 'refused wrapper calls')
