"""Writes tests/golden/prune_cases.npz: magnitude-prune cases for
rigl_magnitude_prune_batched and a schedule trace, computed with the NumPy
restatement of contrib's model_pruning (tests/prune_ref.py).  Seeded and
uncompressed, so a rerun regenerates the file byte-identically:

  python tests/golden/make_golden_prune.py

A case is one batched call: layers L0..L{m-1}, each with raw weights w, its old
bitmap, old threshold and k; the expected new threshold, bitmap and popcounts.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import prune_ref as R  # noqa: E402

F32 = np.float32


def _layer(out, tag, i, w, k, thr_old, decay, rs):
  w = np.asarray(w, F32).reshape(-1)
  n = w.size
  old = (rs.rand(n) < 0.7).astype(np.uint8)
  thr, mask = R.mask_update(w, k, thr_old, decay)
  p = '%s__L%d_' % (tag, i)
  out[p + 'w'] = w
  out[p + 'k'] = np.int64(k)
  out[p + 'thr_old'] = F32(thr_old)
  out[p + 'mask_old'] = R.pack_bits(old)
  out[p + 'thr'] = F32(thr)
  out[p + 'mask'] = R.pack_bits(mask)
  out[p + 'ones_old'] = np.int64(old.sum())
  out[p + 'ones'] = np.int64(mask.sum())


def _case(out, tag, layers, decay, rs):
  """layers: [(w, k, thr_old)]."""
  out[tag + '__n_layers'] = np.int64(len(layers))
  out[tag + '__decay'] = np.float64(decay)
  for i, (w, k, thr_old) in enumerate(layers):
    _layer(out, tag, i, w, k, thr_old, decay, rs)


def gen_cases(rs):
  out = {}
  # random layers, odd sizes (one word, a partial word, a word + 1, a chunk + 1, several chunks)
  rnd = []
  for n, s in ((1, 0.0), (31, 0.5), (33, 0.9), (4097, 0.75), (1000, 0.5), (70001, 0.9), (12288, 0.3)):
    rnd.append((rs.randn(n).astype(F32), R.k_of(n, s), 0.0))
  _case(out, 'random', rnd, 0.0, rs)
  # heavy ties: weights quantised to a few values (either sign), so the k-th value repeats and popcount > k
  q = np.array([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0], F32)
  ties = [(q[rs.randint(0, 7, n)], k, 0.0) for n, k in ((4096, 1000), (5000, 2500), (33, 7), (9000, 1))]
  _case(out, 'ties', ties, 0.0, rs)
  # +-0.0 and denormals: the k-th value is a denormal, a zero (threshold 0 admits every weight), or a normal above them
  tiny = np.array([0.0, -0.0, 1e-45, -1e-45, 3e-42, -7e-41, 1.1754942e-38, -1.17549435e-38], F32)

  def dz(n):
    w = tiny[rs.randint(0, len(tiny), n)].copy()
    big = rs.rand(n) < 0.1
    w[big] = rs.randn(int(big.sum())).astype(F32)
    return w
  den = []
  for n in (64, 3000, 5000):
    w = dz(n)
    a = np.sort(np.abs(w))[::-1]
    nz = int((a > 0).sum())
    for k in (max(1, nz - 3), nz + 5 if nz + 5 <= n else n, n):
      den.append((w, k, 0.0))
  _case(out, 'zeros_denormals', den, 0.0, rs)
  # k == n and k == 1
  ext = []
  for n in (777, 4096, 4100):
    w = rs.randn(n).astype(F32)
    ext += [(w, n, 0.0), (w, 1, 0.0)]
  _case(out, 'k_extremes', ext, 0.0, rs)
  # threshold_decay 0.5 with a non-zero old threshold (above and below the new k-th value), and decay 0 ignoring it
  dec = [(rs.randn(n).astype(F32), R.k_of(n, s), t) for n, s, t in
         ((5000, 0.5, 0.3), (4097, 0.9, 2.5), (33, 0.25, 0.05), (20000, 0.6, 1.0))]
  _case(out, 'decay05', dec, 0.5, rs)
  _case(out, 'decay0_old', dec, 0.0, rs)
  return out


SCHEDULES = {
    # mnist_train_eval.py:320-337 shape: begin/end used for both the pruning and the sparsity-function steps
    'mnist': dict(begin=4, end=40, frequency=4, initial=0.0, target=0.9, exponent=3,
                  layers=(('layer1/weights', 784 * 300), ('layer2/weights', 300 * 100), ('layer3/weights', 100 * 10)),
                  smap={'layer2': 0.45, 'layer3': 0.0}),
    # contrib's defaults: end_pruning_step = -1 (prune forever), sparsity_function 0 .. 100
    'defaults': dict(begin=0, end=-1, sbegin=0, send=100, frequency=10, initial=0.0, target=0.5, exponent=3,
                     layers=(('conv1/weights', 3 * 3 * 3 * 16), ('fc/weights', 64 * 10)), smap={}),
}


def gen_schedule():
  out = {}
  for tag, c in SCHEDULES.items():
    sb, se = c.get('sbegin', c['begin']), c.get('send', c['end'])
    steps = np.arange(0, 131, dtype=np.int64)
    s_all, gates, ks, last = [], [], [], 0
    for t in steps:
      s = R.sparsity(int(t), c['initial'], c['target'], sb, se, c['exponent'])
      s_all.append(s)
      g = R.gate(int(t), last, c['begin'], c['end'], c['frequency'])
      gates.append(g)
      if g:
        last = int(t)
      ks.append([R.k_of(n, R.layer_sparsity(name, s, c['smap'], c['target'])) for name, n in c['layers']])
    p = 'sched_%s__' % tag
    out[p + 'steps'] = steps
    out[p + 's'] = np.array(s_all, F32)
    out[p + 'gate'] = np.array(gates, np.uint8)
    out[p + 'k'] = np.array(ks, np.int64)
  return out


def main():
  rs = np.random.RandomState(20261016)
  cases = {}
  cases.update(gen_cases(rs))
  cases.update(gen_schedule())
  buf = io.BytesIO()
  np.savez(buf, **{k: cases[k] for k in sorted(cases)})   # uncompressed: byte-identical on every run
  with open(os.path.join(HERE, 'prune_cases.npz'), 'wb') as f:
    f.write(buf.getvalue())
  print('prune golden vectors written to', HERE)


if __name__ == '__main__':
  main()
