#!/usr/bin/env python3
"""Golden vectors for the learning-rate schedules, produced by EXECUTING the reference's own set_lr_schedule and
lr_schedule (rigl/imagenet_resnet/imagenet_train_eval.py:280-330, unmodified).

    RIGL_REFERENCE=<checkout of the reference> python tests/golden/make_golden_lr.py

The module's imports (TensorFlow, absl, the TPU estimator) cannot be satisfied offline, so the two function definitions
are taken out of the file's syntax tree and executed in a namespace that holds
  * a stub FLAGS,
  * ``tf``: the few TF calls the two functions make -- tf.where, tf.train.cosine_decay_restarts, tf.logging.info -- over
    ``T``, an fp32 scalar whose operators round once per operation and convert Python numbers to fp32 first, as TF's
    operator overloads do for a float32 tensor.
current_epoch is built as :352-353 do: tf.cast(global_step, tf.float32) / (num_train_images / train_batch_size).

What is NOT executed: tf.train.cosine_decay_restarts itself.  ``cosine_decay_restarts`` below writes out the formula of
TF 1.15's learning_rate_decay.py in fp32 NumPy; its floor(log / log) is undetermined within rounding at a restart, so for
the SGDR cases only steps further than 1e-4 of a cycle length from every restart are recorded (asserted below), and the
tests compare those cases within a bound instead of bit for bit.

The fixture (tests/golden/lr_schedule.npz) is written with fixed zip timestamps: regenerating it gives the same bytes.
"""
import ast
import io
import math
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32

BASE_LR = 0.1
NUM_TRAIN_IMAGES = 1281167
TRAIN_STEPS = 2 ** 26            # the flag's value BEFORE the multiplier: every recorded step lies inside the run
SGDR = dict(sgdr_decay_step=5, sgdr_t_mul=1.5, sgdr_m_mul=.5)          # the flags' defaults (:218-221)
ARCHS = ('resnet', 'mobilenet_v1', 'vgg_16')
# 1.0 and 0.5 keep the warm-up's divisor a power of two (8 and 4 epochs), where (c * x) / d and c * (x / d) are the same
# number; 0.3 (2.4 epochs) is there so that the records pin the ORDER of the warm-up's two operations as well
MULTIPLIERS = (1.0, 0.5, 0.3)
BATCHES = (256, 4096)
RESTART_MARGIN = 1e-4


# ---- the stand-in for the TF calls --------------------------------------------------------------------------------------
def _f(v):
  return v.v if isinstance(v, T) else F(v)


class T:
  """An fp32 scalar tensor: every operator is one fp32 operation; Python numbers become fp32 constants first."""

  def __init__(self, v):
    self.v = F(v)

  def __mul__(self, o): return T(self.v * _f(o))
  def __rmul__(self, o): return T(_f(o) * self.v)
  def __truediv__(self, o): return T(self.v / _f(o))
  def __rtruediv__(self, o): return T(_f(o) / self.v)
  def __add__(self, o): return T(self.v + _f(o))
  def __radd__(self, o): return T(_f(o) + self.v)
  def __sub__(self, o): return T(self.v - _f(o))
  def __rsub__(self, o): return T(_f(o) - self.v)
  def __lt__(self, o): return bool(self.v < _f(o))
  def __le__(self, o): return bool(self.v <= _f(o))


def where(cond, a, b):
  return T(_f(a) if cond else _f(b))


def cosine_decay_restarts(learning_rate, global_step, first_decay_steps, t_mul=2.0, m_mul=1.0, alpha=0.0):
  """TF 1.15 learning_rate_decay.py cosine_decay_restarts, dtype float32 (written out from its documentation, not run)."""
  lr, gs, fds, t, m, a = (_f(v) for v in (learning_rate, global_step, first_decay_steps, t_mul, m_mul, alpha))
  one = F(1.0)
  completed = gs / fds
  if t == one:
    i_restart = np.floor(completed)
    completed = completed - i_restart
  else:
    i_restart = np.floor(np.log(one - completed * (one - t)) / np.log(t))
    sum_r = (one - np.power(t, i_restart)) / (one - t)
    completed = (completed - sum_r) / np.power(t, i_restart)
  m_fac = np.power(m, i_restart)
  cosine_decayed = F(0.5) * m_fac * (one + F(np.cos(np.float64(F(math.pi) * completed))))
  decayed = (one - a) * cosine_decayed + a
  return T(lr * decayed)


def make_tf():
  tf = types.SimpleNamespace()
  tf.where = where
  tf.train = types.SimpleNamespace(cosine_decay_restarts=cosine_decay_restarts)
  tf.logging = types.SimpleNamespace(info=lambda *a, **k: None)
  return tf


# ---- the reference's two functions --------------------------------------------------------------------------------------
def load_reference_functions(ref_root):
  path = os.path.join(ref_root, 'rigl', 'imagenet_resnet', 'imagenet_train_eval.py')
  tree = ast.parse(open(path).read(), path)
  defs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ('set_lr_schedule', 'lr_schedule')]
  assert sorted(d.name for d in defs) == ['lr_schedule', 'set_lr_schedule'], 'the reference file changed'
  ns = {'tf': make_tf(), 'FLAGS': None, 'LR_SCHEDULE': []}
  exec(compile(ast.Module(body=defs, type_ignores=[]), path, 'exec'), ns)   # pylint: disable=exec-used
  return ns


def flags_for(arch, mult, batch, sgdr):
  return types.SimpleNamespace(
      model_architecture=arch, training_steps_multiplier=mult, train_batch_size=batch, base_learning_rate=BASE_LR,
      num_train_images=NUM_TRAIN_IMAGES, use_sgdr=sgdr, train_steps=TRAIN_STEPS, maskupdate_begin_step=0,
      maskupdate_end_step=0, **SGDR)


def epoch32(step, flags):
  steps_per_epoch = flags.num_train_images / flags.train_batch_size                      # :352
  return T(F(step)) / steps_per_epoch                                                    # :353


def boundary_steps(flags, table):
  """For every start epoch of the table: the last step whose fp32 epoch is below it and the first step at or above it."""
  out = []
  spe = flags.num_train_images / flags.train_batch_size
  for _, start in table:
    s = int(start * spe)
    while s > 0 and not epoch32(s, flags) < start:
      s -= 1
    while epoch32(s + 1, flags) < start:
      s += 1
    first = s + 1 if epoch32(s, flags) < start else s      # (start 0: step 0 is the first at or above it, none below)
    out += [max(first - 1, 0), first]
  return out


def sgdr_far_from_restart(step, flags):
  """True when the step's epoch is further than RESTART_MARGIN of a cycle length from every restart (in double)."""
  x = float(epoch32(step, flags).v)
  t, fds = float(F(flags.sgdr_t_mul)), float(F(flags.sgdr_decay_step))
  restart, length = fds, fds                           # the first restart ends cycle 0 (epoch 0 itself is no restart)
  while restart - length <= x:
    if abs(x - restart) <= RESTART_MARGIN * length * t:  # (the longer of the two cycles that meet there)
      return False
    length *= t
    restart += length
  return True


def generate(ref_root):
  ns = load_reference_functions(ref_root)
  cases, rec_case, rec_step, rec_bits = [], [], [], []
  with np.errstate(all='ignore'):                    # the ResNet chain's warm-up divides by its start epoch 0 (never selected)
    for arch in ARCHS:
      for mult in MULTIPLIERS:
        for batch in BATCHES:
          for sgdr in (False, True):
            flags = flags_for(arch, mult, batch, sgdr)
            ns['FLAGS'] = flags
            ns['set_lr_schedule']()
            table = list(ns['LR_SCHEDULE'])
            last = int(table[-1][1] * 1.1 * flags.num_train_images / batch)
            steps = {0, 1, 2 ** 24 + 1}
            steps.update(boundary_steps(flags, table))
            steps.update(int(round(s)) for s in np.logspace(0, math.log10(last), 64))
            if sgdr:
              kept = {s for s in steps if sgdr_far_from_restart(s, flags)}
              assert 0 in kept and len(kept) >= 48, 'too few SGDR steps survive the restart margin'
              steps = kept
            for s in sorted(steps):
              if sgdr:
                assert sgdr_far_from_restart(s, flags)
              lr = ns['lr_schedule'](epoch32(s, flags))
              rec_case.append(len(cases))
              rec_step.append(s)
              rec_bits.append(F(_f(lr)).view(np.uint32))
            cases.append((arch, mult, batch, sgdr))
  return {
      'case_arch': np.array([c[0] for c in cases], dtype='U16'),
      'case_multiplier': np.array([c[1] for c in cases], dtype=np.float64),
      'case_batch': np.array([c[2] for c in cases], dtype=np.int64),
      'case_sgdr': np.array([c[3] for c in cases], dtype=np.bool_),
      'base_learning_rate': np.float64(BASE_LR),
      'num_train_images': np.int64(NUM_TRAIN_IMAGES),
      'train_steps': np.int64(TRAIN_STEPS),
      'sgdr_decay_step': np.float64(SGDR['sgdr_decay_step']),
      'sgdr_t_mul': np.float64(SGDR['sgdr_t_mul']),
      'sgdr_m_mul': np.float64(SGDR['sgdr_m_mul']),
      'rec_case': np.array(rec_case, dtype=np.int32),
      'rec_step': np.array(rec_step, dtype=np.int64),
      'rec_lr_bits': np.array(rec_bits, dtype=np.uint32),
  }


def write_npz(path, arrays):
  """np.savez_compressed with fixed member timestamps (the zip header would otherwise record the time of the run)."""
  with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
    for name in sorted(arrays):
      buf = io.BytesIO()
      np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
      info = zipfile.ZipInfo(name + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
      info.compress_type = zipfile.ZIP_DEFLATED
      info.external_attr = 0o644 << 16
      z.writestr(info, buf.getvalue())


def main():
  ref = os.environ.get('RIGL_REFERENCE') or (sys.argv[1] if len(sys.argv) > 1 else None)
  if not ref or not os.path.isdir(ref):
    sys.exit('usage: RIGL_REFERENCE=<checkout of the reference> make_golden_lr.py')
  out = os.path.join(HERE, 'lr_schedule.npz')
  arrays = generate(ref)
  write_npz(out, arrays)
  print('%d records of %d cases written to %s' % (len(arrays['rec_step']), len(arrays['case_arch']), out))


if __name__ == '__main__':
  main()
