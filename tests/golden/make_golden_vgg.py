#!/usr/bin/env python3
"""Generates tests/golden/vgg_sparsities.json by EXECUTING THE REFERENCE's own
``rigl/sparse_utils.get_sparsities`` (over the NumPy shim in ``tf_shim.py``, as
``make_golden.py`` does) on the VGG-A / VGG-16 / VGG-19 mask tables.

The tables are written out here from rigl/imagenet_resnet/vgg.py:57-200 and
TF-slim's ``layers.repeat`` naming (scope convS, calls convS_1 .. convS_n,
inside tf.variable_scope(vgg_type)); fc8 is a masked 1x1 conv (HWIO).

  python tests/golden/make_golden_vgg.py        # rewrites the fixture
"""
import json
import os
import sys
import types
from collections import OrderedDict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('RIGL_REFERENCE', '/root/reference')
sys.path.insert(0, HERE)

import tf_shim  # noqa: E402

tf_shim.install()
_pkg = types.ModuleType('rigl')
_pkg.__path__ = [os.path.join(REF, 'rigl')]
sys.modules['rigl'] = _pkg

from rigl import sparse_utils as ref_su  # noqa: E402

REPEATS = {'vgg_a': [1, 1, 2, 2, 2], 'vgg_16': [2, 2, 3, 3, 3], 'vgg_19': [2, 2, 4, 4, 4]}
FILTERS = [64, 128, 256, 512, 512]


def vgg_table(vgg_type, width=1.0, num_classes=1000):
  t = OrderedDict()
  cin = 3
  for s, (reps, f) in enumerate(zip(REPEATS[vgg_type], FILTERS)):
    cout = int(f * width)
    for i in range(reps):
      t['%s/conv%d/conv%d_%d/mask:0' % (vgg_type, s + 1, s + 1, i + 1)] = (3, 3, cin, cout)
      cin = cout
  t['%s/fc8/mask:0' % vgg_type] = (1, 1, cin, num_classes)
  return t


def gen():
  runs = []
  for vgg_type in ('vgg_a', 'vgg_16', 'vgg_19'):
    for width in (1.0, 0.5):
      for method in ('erdos_renyi_kernel', 'erdos_renyi', 'random'):
        for s in (0.8, 0.9):
          table = vgg_table(vgg_type, width)
          masks = [tf_shim.Variable(np.ones(shape, np.float32), name[:-len(':0')]) for name, shape in table.items()]
          res = ref_su.get_sparsities(masks, method, s, {})
          runs.append(dict(net=vgg_type, width=width, method=method, default_sparsity=s,
                           names=[m.name for m in masks], shapes=[list(m.shape) for m in masks],
                           sparsities=[float(res[m.name]).hex() for m in masks]))
  return dict(runs=runs)


def main():
  with open(os.path.join(HERE, 'vgg_sparsities.json'), 'w') as f:
    json.dump(gen(), f, indent=1)
  print('golden vectors written to', HERE)


if __name__ == '__main__':
  main()
