"""Shared by the learning-rate schedule tests: the golden records (tests/golden/lr_schedule.npz, written by
tests/golden/make_golden_lr.py from the reference's own lr_schedule), the Schedule each record's flags build, and a plain
NumPy restatement of the reference function with switchable MUTATIONS -- the golden comparison must reject each of them,
which shows that the records can tell the schedules' rounding order and comparison apart."""
import functools
import math
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lr_schedule.npz')


@functools.lru_cache(maxsize=None)
def golden():
  """-> (meta dict, list of cases): a case is (flags dict, steps int64 [k], lr bits uint32 [k])."""
  z = np.load(GOLDEN)
  meta = {k: z[k].item() for k in ('base_learning_rate', 'num_train_images', 'train_steps', 'sgdr_decay_step', 'sgdr_t_mul',
                                    'sgdr_m_mul')}
  cases = []
  for i in range(len(z['case_arch'])):
    sel = z['rec_case'] == i
    flags = dict(arch=str(z['case_arch'][i]), multiplier=float(z['case_multiplier'][i]), batch=int(z['case_batch'][i]),
                 sgdr=bool(z['case_sgdr'][i]))
    cases.append((flags, z['rec_step'][sel], z['rec_lr_bits'][sel]))
  return meta, cases


def schedule_for(flags, meta):
  from rigl_amd import schedules
  return schedules.imagenet_lr_schedule(
      meta['base_learning_rate'], flags['batch'], num_train_images=meta['num_train_images'],
      model_architecture=flags['arch'], training_steps_multiplier=flags['multiplier'], use_sgdr=flags['sgdr'],
      sgdr_decay_step=meta['sgdr_decay_step'], sgdr_t_mul=meta['sgdr_t_mul'], sgdr_m_mul=meta['sgdr_m_mul'],
      train_steps=meta['train_steps'])


def sgdr_cycle(flags, meta, step):
  """(lr0, m_fac) of the SGDR cycle that holds ``step``, in double: the scale of the cosine bound."""
  x = float(F(step) / F(meta['num_train_images'] / flags['batch']))
  t, fds = float(F(meta['sgdr_t_mul'])), float(F(meta['sgdr_decay_step']))
  i, end, length = 0, fds, fds
  while x >= end:
    length *= t
    end += length
    i += 1
  return meta['base_learning_rate'] * (flags['batch'] / 256.0), float(F(meta['sgdr_m_mul'])) ** i


MUTATIONS = ('le_in_chain', 'warmup_divides_first', 'product_in_fp32')


def reference_chain(flags, meta, step, mutation=None):
  """The non-SGDR lr_schedule of imagenet_train_eval.py:317-330 at ``step`` -> np.float32, optionally with one mutation."""
  assert mutation is None or mutation in MUTATIONS
  if flags['arch'].startswith('mobilenet'):
    table = [(1.0, 8), (0.1, 40), (0.01, 75), (0.001, 95), (.0003, 120)]
  else:
    table = [(1.0, 0), (0.1, 30), (0.01, 70), (0.001, 90), (.0001, 120)]
  if flags['multiplier'] != 1.0:
    table = [(x, y * flags['multiplier']) for x, y in table]
  spe = meta['num_train_images'] / flags['batch']
  x = F(step) / F(spe)
  scaled_lr = meta['base_learning_rate'] * (flags['batch'] / 256.0)
  with np.errstate(all='ignore'):
    if mutation == 'warmup_divides_first':
      rate = F(scaled_lr * table[0][0]) * (x / F(table[0][1]))
    else:
      rate = F(scaled_lr * table[0][0]) * x / F(table[0][1])
  for k, (mult, start) in enumerate(table):
    below = x <= F(start) if mutation == 'le_in_chain' else x < F(start)
    value = F(scaled_lr * mult)
    if mutation == 'product_in_fp32' and k > 0:
      value = F(F(scaled_lr) * F(mult))               # the product taken in fp32 instead of in Python doubles
    rate = rate if below else value
  return F(rate)


def bits(v):
  return int(np.asarray(v, dtype=np.float32).view(np.uint32))


INT32_MAX = 2 ** 31 - 1
PI = math.pi
