"""VGG-A / VGG-16 / VGG-19 (rigl/imagenet_resnet/vgg.py), the parts that need no device: the mask tables (names, HWIO
shapes, creation order), the sparsity distributions against the reference's own get_sparsities
(tests/golden/vgg_sparsities.json, written by tests/golden/make_golden_vgg.py), the arguments the workload refuses, and
the declared C ABI of the conv + ReLU entry points."""
import json
import os
import re
from collections import OrderedDict, namedtuple

import pytest

torch = pytest.importorskip('torch')

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, 'tests', 'golden')

# Written out by hand from vgg.py:57-200 (network_cfg, 64/128/256/512/512 filters, layers.repeat scopes) -- independent
# of rigl_amd.workloads.shapes.
_VGG_16 = [('conv1/conv1_1', 3, 64), ('conv1/conv1_2', 64, 64),
           ('conv2/conv2_1', 64, 128), ('conv2/conv2_2', 128, 128),
           ('conv3/conv3_1', 128, 256), ('conv3/conv3_2', 256, 256), ('conv3/conv3_3', 256, 256),
           ('conv4/conv4_1', 256, 512), ('conv4/conv4_2', 512, 512), ('conv4/conv4_3', 512, 512),
           ('conv5/conv5_1', 512, 512), ('conv5/conv5_2', 512, 512), ('conv5/conv5_3', 512, 512)]
_VGG_A = [('conv1/conv1_1', 3, 64), ('conv2/conv2_1', 64, 128),
          ('conv3/conv3_1', 128, 256), ('conv3/conv3_2', 256, 256),
          ('conv4/conv4_1', 256, 512), ('conv4/conv4_2', 512, 512),
          ('conv5/conv5_1', 512, 512), ('conv5/conv5_2', 512, 512)]
_VGG_19 = [('conv1/conv1_1', 3, 64), ('conv1/conv1_2', 64, 64),
           ('conv2/conv2_1', 64, 128), ('conv2/conv2_2', 128, 128),
           ('conv3/conv3_1', 128, 256), ('conv3/conv3_2', 256, 256), ('conv3/conv3_3', 256, 256), ('conv3/conv3_4', 256, 256),
           ('conv4/conv4_1', 256, 512), ('conv4/conv4_2', 512, 512), ('conv4/conv4_3', 512, 512), ('conv4/conv4_4', 512, 512),
           ('conv5/conv5_1', 512, 512), ('conv5/conv5_2', 512, 512), ('conv5/conv5_3', 512, 512), ('conv5/conv5_4', 512, 512)]
_TABLES = {'vgg_a': _VGG_A, 'vgg_16': _VGG_16, 'vgg_19': _VGG_19}


def _expected(vgg_type, width, num_classes=1000, prune_last_layer=True):
  out = []
  for name, cin, cout in _TABLES[vgg_type]:
    c_in = 3 if cin == 3 else int(cin * width)
    out.append(('%s/%s/mask:0' % (vgg_type, name), (3, 3, c_in, int(cout * width))))
  if prune_last_layer:
    out.append(('%s/fc8/mask:0' % vgg_type, (1, 1, int(512 * width), num_classes)))
  return out


@pytest.mark.parametrize('vgg_type', ['vgg_a', 'vgg_16', 'vgg_19'])
@pytest.mark.parametrize('width', [1.0, 0.5])
def test_mask_table(vgg_type, width):
  from rigl_amd.workloads import shapes as WS
  assert list(WS.vgg_masks(vgg_type, width=width).items()) == _expected(vgg_type, width)
  assert list(WS.vgg_masks(vgg_type, prune_last_layer=False, num_classes=10, width=width).items()) == \
      _expected(vgg_type, width, 10, False)


@pytest.mark.parametrize('vgg_type', ['vgg_a', 'vgg_16'])
def test_model_creates_the_table_in_order(vgg_type):
  from rigl_amd import variables as V
  from rigl_amd.workloads import vgg
  g = V.Graph('cpu')
  vgg.VGG(vgg_type, num_classes=10, width=0.5, weight_decay=5e-4, graph=g)
  got = [(l.mask.name, tuple(l.weights.shape)) for l in g.layers if l.mask is not None]
  assert got == _expected(vgg_type, 0.5, 10)
  assert all(l.weights.weight_decay == 5e-4 for l in g.layers)


def test_sparsities_match_reference():
  from rigl_amd import sparse_utils as SU
  from rigl_amd.workloads import shapes as WS
  M = namedtuple('M', 'name shape')
  data = json.load(open(os.path.join(G, 'vgg_sparsities.json')))
  seen = set()
  for r in data['runs']:
    table = WS.vgg_masks(r['net'], width=r['width'])
    assert list(table.keys()) == r['names'] and [list(s) for s in table.values()] == r['shapes']
    got = SU.get_sparsities([M(n, s) for n, s in table.items()], r['method'], r['default_sparsity'], {})
    for name, ref_hex in zip(r['names'], r['sparsities']):
      assert float(got[name]) == float.fromhex(ref_hex), (r['net'], r['method'], name)
    seen.add((r['net'], r['width'], r['method'], r['default_sparsity']))
  assert len(seen) == 3 * 2 * 3 * 2


def test_refused_arguments():
  from rigl_amd import variables as V
  from rigl_amd.workloads import vgg
  for init in ('sparse', 'random_zeros'):
    with pytest.raises(NotImplementedError):
      vgg.VGG('vgg_16', graph=V.Graph('cpu'), init_method=init)
  with pytest.raises(NotImplementedError):
    vgg.VGG('vgg_16', graph=V.Graph('cpu'), precision='float32')
  for width in (0.3, 0.1, 1.01):
    with pytest.raises(ValueError):
      vgg.VGG('vgg_16', graph=V.Graph('cpu'), width=width)
  with pytest.raises(ValueError):
    vgg.VGG('vgg_11', graph=V.Graph('cpu'))
  m = vgg.VGG('vgg_a', num_classes=10, width=0.25, graph=V.Graph('cpu'))
  for h, w in ((24, 32), (32, 40), (8, 16)):
    with pytest.raises(ValueError):
      m(torch.zeros(2, h, w, 3, dtype=torch.bfloat16))
  with pytest.raises(NotImplementedError):
    m(torch.zeros(2, 32, 32, 3, dtype=torch.float32))
  # conv1_2's output at 224 x 224 is 224 * 224 * 64 bf16 per image: 2^30 elements near batch 334
  big = vgg.VGG('vgg_16', num_classes=10, graph=V.Graph('cpu'))
  with pytest.raises(ValueError, match='2\\^30'):
    big._check_input(torch.empty(335, 224, 224, 3, dtype=torch.bfloat16, device='meta'))
  big._check_input(torch.empty(334, 224, 224, 3, dtype=torch.bfloat16, device='meta'))


def test_vgg16_flops_from_shapes():
  from rigl_amd.workloads import shapes as WS
  fwd, dgrad, fc8 = WS.vgg_macs_per_image('vgg_16')
  assert fwd == 15346630656 and fwd - dgrad == 3 * 64 * 9 * 224 * 224 and fc8 == 512 * 1000
  assert abs(128 * 2 * (2 * fwd + dgrad) / 1e12 - 11.76) < 0.01


def test_c_abi_declared():
  h = open(os.path.join(ROOT, 'include', 'rigl_hip.h')).read()
  from rigl_amd import _lib
  for name in ('rigl_masked_conv2d_fwd_relu', 'rigl_masked_conv2d_bwd_relu', 'rigl_conv2d_fwd_takes_relu_epilogue',
               'rigl_conv2d_bwd_takes_relu_epilogue', 'rigl_relu_fwd', 'rigl_relu_bwd', 'rigl_global_avgpool_bwd_relu'):
    assert re.search(r'\b%s\(' % name, h), name
    assert name in _lib.SIGNATURES, name
