#!/usr/bin/env python3
"""Generates tests/golden/adam_cases.npz by EXECUTING THE REFERENCE with an Adam
inner optimizer.

The reference wraps ``tf.train.AdamOptimizer`` in its ImageNet (``--use_adam``)
and MNIST (``--optimizer=adam``) drivers.  This script drives the reference's
own, unmodified ``SparseRigLOptimizerBase`` / ``SparseSETOptimizerBase`` (through
``make_golden.py`` and the NumPy TensorFlow shim, both imported as they are)
with a shim ``AdamOptimizer``: the fp32 restatement of TF's ``ApplyAdam``
(training_ops.cc, non-Nesterov), slots ``m`` and ``v``, and the two beta-power
accumulators advanced once per ``apply_gradients`` (``_finish``).

  python tests/golden/make_golden_adam.py   # rewrites adam_cases.npz

Recorded:
  single_<tag>__*  one mask update with both slots pre-filled at random, RigL
                   (slot reset = dense_grad * initial_acc_scale, acc 0 / 0.5) and
                   SET (slot reset = 0), reinit_when_same off / on.
  traj_<tag>__*    24 minimize() calls of the reference test's toy problem
                   (make_golden._fc_problem(12, 20, 'rigl', 1, 17, 4, 0.4,
                   'cosine')): w, mask, m, v, global step and beta powers after
                   every call, initial_acc_scale 0 and 0.5.
"""
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as MG  # noqa: E402  (installs the TF shim, imports the reference)
import tf_shim  # noqa: E402

F32 = np.float32
V = tf_shim.Variable
_Inner = MG.shim_opt.GradientDescentOptimizer.__bases__[0]


class AdamOptimizer(_Inner):
  """tf.train.AdamOptimizer (ApplyAdam, use_nesterov=False) in fp32 NumPy:
    alpha = (lr * sqrt(1 - beta2_power)) / (1 - beta1_power)
    m += (g - m) * (1 - beta1);  v += (g*g - v) * (1 - beta2)
    w -= (m * alpha) / (sqrt(v) + epsilon)
  every operation rounded to fp32; the beta powers start at beta1 / beta2 and
  are multiplied by them once per apply, after every variable (_finish)."""

  def __init__(self, grad_fn, learning_rate=0.001, beta1=0.9, beta2=0.999,
               epsilon=1e-8):
    super().__init__(grad_fn, 'Adam')
    self._lr = F32(learning_rate)
    self._beta1 = F32(beta1)
    self._beta2 = F32(beta2)
    self._eps = F32(epsilon)
    self.beta1_power = F32(beta1)
    self.beta2_power = F32(beta2)

  def get_slot_names(self):
    return ['m', 'v']

  def get_slot(self, var, name):
    return self._slots[(var.name, name)]

  def _create_slots(self, var_list):
    for v in var_list:
      for s in ('m', 'v'):
        key = (v.name, s)
        if key not in self._slots:
          self._slots[key] = V(np.zeros_like(v.value), v.name[:-2] + '/Adam_' + s)

  def _apply_one(self, g, v):
    m = self._slots[(v.name, 'm')]
    s = self._slots[(v.name, 'v')]
    g = g.astype(F32)
    alpha = F32(F32(self._lr * F32(np.sqrt(F32(F32(1) - self.beta2_power)))) /
                F32(F32(1) - self.beta1_power))
    omb1 = F32(F32(1) - self._beta1)
    omb2 = F32(F32(1) - self._beta2)
    m.value = (m.value + ((g - m.value).astype(F32) * omb1).astype(F32)).astype(F32)
    s.value = (s.value + (((g * g).astype(F32) - s.value).astype(F32) * omb2).astype(F32)).astype(F32)
    den = (np.sqrt(s.value).astype(F32) + self._eps).astype(F32)
    v.value = (v.value - ((m.value * alpha).astype(F32) / den).astype(F32)).astype(F32)

  def _finish(self):
    self.beta1_power = F32(self.beta1_power * self._beta1)
    self.beta2_power = F32(self.beta2_power * self._beta2)

  def apply_gradients(self, grads_and_vars, global_step=None, name=None):
    op = super().apply_gradients(grads_and_vars, global_step=global_step, name=name)

    def fn():
      op.run()
      self._finish()

    return tf_shim.LazyOp(fn)


def _single(rs, method, acc_scale, reinit, shape=(16, 24), frac=0.3):
  """One _get_update_op of the reference base on one layer, Adam slots pre-filled."""
  tf_shim.STORE.reset()
  n = int(np.prod(shape))
  w = rs.randn(*shape).astype(F32)
  mask = (rs.rand(*shape) < 0.5).astype(F32)
  g = rs.randn(*shape).astype(F32)
  m0 = rs.randn(*shape).astype(F32)
  v0 = np.abs(rs.randn(*shape)).astype(F32)
  score_drop = np.abs(mask * w).astype(F32) + (rs.randn(*shape) * 1e-5).astype(F32)
  score_grow = np.abs(g).astype(F32)
  score_grow.reshape(-1)[rs.choice(n, n // 8, replace=False)] = F32(0.5)   # ties at the grow threshold
  wv = V(w.copy(), 'layer/weights')
  mv = V(mask.copy(), 'layer/mask')
  inner = AdamOptimizer(lambda vl: [])
  inner._create_slots([wv])
  inner.get_slot(wv, 'm').value = m0.copy()
  inner.get_slot(wv, 'v').value = v0.copy()
  if method == 'rigl':
    opt = MG.RefRigL(inner, 0, 100, 1, drop_fraction=0.1, initial_acc_scale=acc_scale)
    opt._weight2masked_grads = {wv.name: g.copy()}
  else:
    opt = MG.RefSET(inner, 0, 100, 1, drop_fraction=0.1)
  opt._ws, opt._ms = [wv], [mv]
  opt.drop_fraction = F32(frac)
  opt._global_step = V(np.int64(0), 'global_step', dtype=np.int64)
  opt._get_update_op(score_drop, score_grow, mv, wv, reinit_when_same=reinit)
  return dict(mask=mask, w=w, dense_grad=g, m=m0, v=v0, score_drop=score_drop, score_grow=score_grow,
              frac=F32(frac), acc_scale=F32(acc_scale), reinit=np.int32(reinit),
              momreset=np.int32(1 if method == 'rigl' else 0),
              new_mask=mv.value.copy(), new_w=wv.value.copy(),
              new_m=inner.get_slot(wv, 'm').value.copy(), new_v=inner.get_slot(wv, 'v').value.copy())


def gen_single():
  rs = np.random.RandomState(2024)
  out = {}
  for method, acc in [('rigl', 0.0), ('rigl', 0.5), ('set', 0.0)]:
    for reinit in (False, True):
      tag = '%s_acc%g_reinit%d' % (method, acc, int(reinit))
      for k, v in _single(rs, method, acc, reinit).items():
        out['single_%s__%s' % (tag, k)] = v
  return out


def gen_trajectory(lr=0.01):
  out = {}
  for tag, acc in [('acc0', 0.0), ('acc05', 0.5)]:
    opt, io_, wv, mv, gs = MG._fc_problem(12, 20, 'rigl', 1, 17, 4, 0.4, anneal='cosine', seed=3, acc_scale=acc)
    adam = AdamOptimizer(io_._grad_fn, learning_rate=lr)
    opt._optimizer = adam
    MG._noise_inject(None)
    adam._create_slots([wv])
    rec = dict(w=[wv.value.copy()], mask=[mv.value.copy()], m=[], v=[], gs=[0], bp=[], frac=[])
    for _ in range(24):
      tf_shim.run_op(opt.minimize(None, gs))
      rec['w'].append(wv.value.copy())
      rec['mask'].append(mv.value.copy())
      rec['m'].append(adam.get_slot(wv, 'm').value.copy())
      rec['v'].append(adam.get_slot(wv, 'v').value.copy())
      rec['gs'].append(int(gs.value))
      rec['bp'].append(np.array([adam.beta1_power, adam.beta2_power], F32))
      rec['frac'].append(F32(opt.drop_fraction))
    out['traj_%s__w' % tag] = np.stack(rec['w'])
    out['traj_%s__mask' % tag] = np.stack(rec['mask'])
    out['traj_%s__m' % tag] = np.stack(rec['m'])
    out['traj_%s__v' % tag] = np.stack(rec['v'])
    out['traj_%s__gs' % tag] = np.array(rec['gs'], np.int64)
    out['traj_%s__bp' % tag] = np.stack(rec['bp'])
    out['traj_%s__frac' % tag] = np.array(rec['frac'], F32)
    out['traj_%s__acc_scale' % tag] = F32(acc)
    out['traj_%s__lr' % tag] = F32(lr)
  return out


def main():
  cases = {}
  cases.update(gen_single())
  cases.update(gen_trajectory())
  buf = io.BytesIO()
  np.savez(buf, **{k: cases[k] for k in sorted(cases)})   # uncompressed: byte-identical on every run
  with open(os.path.join(HERE, 'adam_cases.npz'), 'wb') as f:
    f.write(buf.getvalue())
  print('adam golden vectors written to', HERE)


if __name__ == '__main__':
  main()
