"""Dropout without a GPU: the reference (tests/dropout_ref.py) against hand cases and against mutants of itself, the host
logic of the WideResNet's ``droprate``, and the argument checks of the C ABI (nothing here touches a device)."""
import ctypes
import math

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from oracle import tf_random as TR  # noqa: E402
from tests import dropout_ref as R  # noqa: E402

N, SEED0 = 65536, 12345


@pytest.fixture(scope='module')
def masks():
  return [R.keep_mask(N, 0.3, SEED0, s) for s in range(4)]


def test_rate_zero_keeps_everything_unchanged():
  x = torch.randn(1000).to(torch.bfloat16)
  y, bits = R.expected_fwd(x, 0.0, SEED0, 3)
  assert R.n_differing(y, x) == 0
  assert np.array_equal(bits, np.full(125, 0xFF, np.uint8))


def test_kept_fraction_is_one_minus_rate(masks):
  # binomial: sigma = sqrt(0.3 * 0.7 / 65536) = 0.0018; 4 sigma = 0.0072
  for m in masks:
    assert abs(float(m.mean()) - 0.7) <= 0.0072, float(m.mean())


def test_consecutive_steps_draw_different_masks(masks):
  # independent masks differ where exactly one keeps: 2 * 0.7 * 0.3 = 42 %
  for a, b in zip(masks, masks[1:]):
    assert float((a != b).mean()) > 0.35


def test_high_rate_keeps_almost_nothing():
  assert float(R.keep_mask(N, 0.999, SEED0, 0).mean()) < 0.003


def test_kept_values_are_scaled_and_dropped_ones_are_plus_zero():
  x = torch.full((64,), 3.0)
  y, bits = R.expected_fwd(x, 0.5, SEED0, 0)
  keep = R.unpack_bits(bits, 64)
  assert 0 < keep.sum() < 64
  assert torch.equal(y[torch.from_numpy(keep)], torch.full((int(keep.sum()),), 6.0))
  assert int(y[torch.from_numpy(~keep)].view(torch.int32).abs().sum()) == 0
  dy = torch.full((64,), -1.0)
  assert torch.equal(R.expected_bwd(dy, bits, 0.5), torch.where(torch.from_numpy(keep), torch.tensor(-2.0), torch.tensor(0.0)))


def test_seed_pair_wraps_to_int32():
  assert np.array_equal(R.keep_mask(64, 0.3, SEED0 + (1 << 32), (1 << 31)), R.keep_mask(64, 0.3, SEED0, -(1 << 31)))


# ---- mutants of the reference: each is rejected by the comparison that is there to catch it ------------------------
def test_mutant_strict_comparison_is_caught_on_a_tie():
  u = TR.stateless_random_uniform(64, SEED0, 0)
  rate = float(u[5])                                  # a rate that element 5 meets exactly
  assert 0.0 < rate < 1.0
  keep = R.keep_mask(64, rate, SEED0, 0)
  assert keep[5]                                      # >= keeps the tie
  mutant = u > np.float32(rate)
  assert not mutant[5] and not np.array_equal(R.pack_bits(keep), R.pack_bits(mutant))


def test_mutant_msb_first_bit_order_is_caught():
  keep = np.array([1, 0, 0, 0, 0, 0, 0, 0, 1], bool)
  assert R.pack_bits(keep).tolist() == [0x01, 0x01]   # LSB first, spare bits 0
  assert np.packbits(keep, bitorder='big').tolist() == [0x80, 0x80]
  assert np.array_equal(R.unpack_bits(R.pack_bits(keep), 9), keep)
  m = R.keep_mask(N, 0.3, SEED0, 0)
  assert not np.array_equal(R.pack_bits(m), np.packbits(m, bitorder='big'))


def test_mutant_multiply_by_zero_is_caught_on_a_dropped_nan():
  keep = R.keep_mask(64, 0.5, SEED0, 0)
  i = int(np.flatnonzero(~keep)[0])
  for special in (float('nan'), float('inf'), -float('inf'), -0.0):
    x = torch.ones(64)
    x[i] = special
    y, _ = R.expected_fwd(x, 0.5, SEED0, 0)
    assert int(y[i].view(torch.int32)) == 0             # +0, bit for bit
    mutant = (x * torch.tensor(R.f32_scale(0.5))) * torch.from_numpy(keep).float()
    assert R.n_differing(y, mutant) >= 1


def test_mutant_bf16_scale_is_caught():
  x = torch.ones(64)
  y, bits = R.expected_fwd(x, 0.3, SEED0, 0)
  s_bf16 = torch.tensor(R.f32_scale(0.3)).to(torch.bfloat16).float()
  assert float(s_bf16) != float(R.f32_scale(0.3))
  mutant = torch.where(torch.from_numpy(R.unpack_bits(bits, 64)), x * s_bf16, torch.zeros(64))
  assert R.n_differing(y, mutant) >= 1


# ---- host logic ------------------------------------------------------------------------------------------------------
def _model(**kw):
  from rigl_amd import variables as V
  from rigl_amd.workloads import wide_resnet
  return wide_resnet.WideResNet(V.Graph('cpu'), depth=10, width=1, **kw)


@pytest.mark.parametrize('rate', [-0.1, 1.0, float('nan')])
def test_droprate_outside_range_raises(rate):
  with pytest.raises(ValueError):
    _model(droprate=rate)


def test_default_is_no_dropout_and_no_state():
  m = _model()
  assert m.droprate == 0.0 and m.dropout_state is None


def test_dropout_seed0_is_pinned_per_block(monkeypatch):
  monkeypatch.delenv('PYTHONHASHSEED', raising=False)   # (a fixed hash seed selects the interpreter's own hash(), as for the mask update)
  m = _model(droprate=0.3, dropout_seed=7)
  assert int(m.dropout_state.step) == 0 and m.dropout_state.step.dtype == torch.int32
  scope = m.blocks[0]['conv1'].scope
  assert scope == 'resnet_model/conv_2_0_1'
  want = TR.tf_seed_pair(7, TR.python_str_hash(scope + '/dropout', 0), 0)[0]
  assert m.dropout_seed0(0) == want == -1201226755
  seeds = [m.dropout_seed0(i) for i in range(len(m.blocks))]
  assert len(set(seeds)) == len(seeds) == 3
  assert all(-(1 << 31) <= s < (1 << 31) for s in seeds)
  assert _model(droprate=0.3).dropout_seed0(0) == want - 7


def test_dropout_is_identity_when_not_training_or_rate_zero():
  from rigl_amd.workloads import nn as gnn
  x = torch.ones(8)
  assert gnn.dropout(x, 0.3, 1, gnn.DropoutState('cpu'), is_training=False) is x
  assert gnn.dropout(x, 0.0, 1, gnn.DropoutState('cpu'), is_training=True) is x


def test_ops_refuse_cpu_tensors():
  from rigl_amd import ops
  step = torch.zeros(1, dtype=torch.int32)
  for call in (lambda: ops.dropout_fwd(torch.ones(8), 0.3, 1, step),
               lambda: ops.dropout_bwd(torch.ones(8), torch.zeros(1, dtype=torch.uint8), 0.3),
               lambda: ops.dropout_advance(step)):
    with pytest.raises(Exception) as ei:
      call()
    assert 'GPU' in str(ei.value)


# ---- C ABI: argument errors are reported before anything touches a device ---------------------------------------------
def test_abi_argument_errors():
  from rigl_amd import _lib
  lib = _lib.load()
  for name in ('rigl_dropout_fwd', 'rigl_dropout_bwd', 'rigl_dropout_advance'):
    assert name in _lib.SIGNATURES and getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
  assert lib.rigl_dropout_fwd(None, None, None, 8, 0, 0.3, 0, None, None) == _lib.RIGL_EINVAL
  assert b'rigl_dropout_fwd' in lib.rigl_last_error()
  assert lib.rigl_dropout_bwd(None, None, None, 8, 0, 0.3, None) == _lib.RIGL_EINVAL
  assert b'rigl_dropout_bwd' in lib.rigl_last_error()
  assert lib.rigl_dropout_advance(None, None) == _lib.RIGL_EINVAL
  assert b'rigl_dropout_advance' in lib.rigl_last_error()
  fake = ctypes.c_void_p(256)                            # never dereferenced: the rate is refused first
  for rate in (1.0, -0.1, math.nan):
    assert lib.rigl_dropout_fwd(fake, fake, fake, 8, 0, rate, 0, fake, None) == _lib.RIGL_EINVAL
    assert b'rate' in lib.rigl_last_error()
    assert lib.rigl_dropout_bwd(fake, fake, fake, 8, 1, rate, None) == _lib.RIGL_EINVAL
  assert lib.rigl_dropout_fwd(fake, fake, fake, 8, 2, 0.3, 0, fake, None) == _lib.RIGL_EINVAL       # dtype
  assert lib.rigl_dropout_fwd(None, None, None, 0, 0, 0.3, 0, None, None) == _lib.RIGL_OK            # n == 0: no launch
  assert lib.rigl_dropout_bwd(None, None, None, 0, 1, 0.3, None) == _lib.RIGL_OK
