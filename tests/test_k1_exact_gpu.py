"""Every K1 conv entry point BIT-EXACTLY on integer operands, with guard bands, through tests/k1_exact.py (one subprocess
per case set, each under its own timeout; the runner walks the kernel-selection settings in-process through ops.tune_set
and stops at the first mismatch).

The tolerance suite (test_k1_parity_gpu.py: Gaussian operands, 2^-8 |ref| + 1e-5 sum|a||b|) cannot tell round-to-nearest-even
from round-half-away, cannot see a term below its tolerance, and never looks outside the output tensor.  Here the operands
are small integers times a power-of-two unit with sum|a||b| <= 2^24 units, so fp32 accumulation is exact in any order and
the expected BITS follow from tests/convref.py's fp64 result and the one documented final rounding (tests/exactref.py) --
every body under every setting must produce them, in a 'low' regime (nothing rounds: the statistics partials must add up
to the exact totals) and a 'round' regime (>= 5 % of the outputs are exact bf16 ties), into outputs carved from a
sentinel-filled buffer: both guards intact, no element left unwritten.

The sets wrn, mlp and odd (k1_check.WRN_CASES / MLP_CASES / ODD_CASES) carry this to the small-channel layers: WideResNet-22's
16 / 32 / 64-channel convs, strided 3x3 with TF SAME padding, strided 1x1 skips and stem; the MNIST MLP's dense layers and
the 10-column heads, which ordinary dispatch sends to the direct kernels of conv_ref.hip; the explicit im2col and tiny-Cin
paths.  There dX is wanted for every shape (the direct dgrad and the host fallbacks of ops.conv_dgrad / ops.conv_bwd), every
wrapper form a shape does not take is asserted REFUSED with its outputs left all sentinel (verdict field "refused"), and the
direct kernels run as forms of their own through force_ref=True (for `small` too); tests/test_exact_small_channel_cpu.py
holds the conditions, mutants and workload shapes of these sets without a GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, timeout):
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'k1_exact.py')] + args, capture_output=True, text=True,
                     timeout=timeout)
  lines = [l for l in r.stdout.splitlines() if l.startswith('{')]
  assert lines, 'no verdict line; stdout tail: %s\nstderr tail: %s' % (r.stdout[-2000:], r.stderr[-3000:])
  out = json.loads(lines[-1])
  print(lines[-1])
  assert r.returncode == 0 and out['ok'], '%s\n%s' % (out, r.stdout[-3000:])
  assert out['diff_bits'] == 0 and out['guards'] == 'intact' and out['unwritten'] == 0
  assert out['regimes'] == ['low', 'round']
  # the input conditions the runner asserted per case, once more on its summary
  assert out['conditions']['max_sum_ab'] <= 2 ** 24
  if args[1] != 'f32':                               # (fp32 outputs do not round: the tie shares are not asserted there)
    assert out['conditions']['min_ties'] >= 0.05 and out['conditions']['min_ties_one_way'] >= 0.02
  return out


# set, cases, settings, timeout (s)
SETS = [
    ('small', 12, 7, 900),          # the PP_SETTINGS of test_k1_parity_gpu.py
    ('pp', 12, 7, 900),
    ('stem', 6, 2, 600),            # default / stem_direct = 0
    ('c3', 6, 2, 600),              # default / c3x3 = 0
    ('bs', 12, 2, 900),             # default / bwdslice = 0
    ('rs', 13, 3, 900),             # rowstream = 2 / default / 0
    ('vgg', 10, 2, 1200),           # with and without the fused ReLU
    ('dw', 17, 1, 600),             # test_k3_k1_gpu.py's depthwise cases
    ('f32', 13, 1, 600),            # the fp32 twin, dense and masked
    ('wrn', 10, 2, 600),            # WideResNet-22's layers: default / all-generic; dX and every wrapper form on every shape
    ('mlp', 6, 1, 600),             # dense layers and heads on the direct kernels (no knob reaches them)
    ('odd', 10, 2, 600),            # ragged shapes, cin / cout % 8 != 0: im2col, tiny Cin, the host fallbacks
]
FULL = ('wrn', 'mlp', 'odd')        # the sets that assert the refusals of the forms a shape does not take


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('name,cases,settings,timeout', SETS, ids=[s[0] for s in SETS])
def test_exact_bits_and_guard_bands(name, cases, settings, timeout):
  out = _run(['--set', name], timeout)
  assert out['cases'] == cases and out['settings'] == settings
  assert (out['refused'] > 0) == (name in FULL)


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
@pytest.mark.parametrize('name,cases,settings,timeout', SETS, ids=[s[0] for s in SETS])
def test_exact_bits_on_an_exact_guarded_poisoned_workspace(name, cases, settings, timeout):
  """The same walks with --workspace exact (tests/wsguard.py): every scratch request exactly as long as the size query
  said, between two 1 MiB guards, pre-filled with 0x00 and then 0xFF -- the expected bits do not depend on the summation
  order, so they hold whether a layer splits or not, and a query that under-reports, a kernel that reads scratch it did
  not initialise or a store outside the declared bytes all show.  Every set is walked in full, vgg included (both halves,
  VGG16_SHAPES and C3_SHAPES: the fp64 references are made once per case and shared by the poisons, so the second poison
  costs kernel time only).  The batch-128 sets are not repeated here."""
  out = _run(['--set', name, '--workspace', 'exact'], timeout)
  assert out['cases'] == cases and out['settings'] == settings
  ws = out['workspace']
  assert ws['mode'] == 'exact' and ws['poisons'] == ['0x00', '0xFF']
  assert ws['guards'] == 'intact' and ws['requests'] > 0
  assert 0 <= ws['max_used'] <= ws['max_bytes']


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_resnet50_layer_shapes_at_batch_128():
  """The 23 distinct ResNet-50 conv shapes at the benchmarked batch: default selection and the all-generic setting."""
  out = _run(['--set', 'resnet50', '--batch', '128'], 2400)
  assert out['cases'] == 23 and out['settings'] == 2


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_mobilenet_v1_layer_shapes_at_batch_128():
  """MobileNet-v1's stem, pointwise layers and final_dense at batch 128: default, rowstream = 2 and all-generic."""
  out = _run(['--set', 'mobilenet_v1', '--batch', '128'], 2400)
  assert out['cases'] == 11 and out['settings'] == 3


@pytest.mark.skipif(not torch.cuda.is_available(), reason='needs a GPU')
def test_mobilenet_v1_depthwise_layers_at_batch_128():
  """The depthwise layers of MobileNet-v1's 13 blocks at batch 128 (nine distinct shapes): fwd (+ statistics), dgrad, wgrad."""
  out = _run(['--set', 'dw128', '--batch', '128'], 1200)
  assert out['cases'] == 9 and out['settings'] == 1
