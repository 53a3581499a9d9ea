"""TEST INFRASTRUCTURE: the reference of the dropout kernels (rigl_dropout_fwd / rigl_dropout_bwd), built from the oracle's
stateless uniform stream (oracle/tf_random.py) and torch-CPU arithmetic.

  u       = tf.random.stateless_uniform([n], seed=[seed0, step], float32)
  keep[i] = u[i] >= f32(rate)
  scale   = f32(1) / (f32(1) - f32(rate))
  y[i]    = keep[i] ? (x[i].float() * scale).to(dtype) : +0          (a select: a dropped NaN / inf / -0 gives +0)
  bits    : byte i / 8, bit i % 8 (LSB first) = keep[i]; the unused high bits of the last byte are 0
  dx[i]   = bit[i] ? (dy[i].float() * scale).to(dtype) : +0
"""
import numpy as np
import torch

from oracle import tf_random as TR


def f32_scale(rate):
  return np.float32(1.0) / (np.float32(1.0) - np.float32(rate))


def keep_mask(n, rate, seed0, step):
  """bool [n]; seed0 / step are wrapped to int32 like the reference's seed pair."""
  s0, s1 = TR.tf_seed_pair(0, int(seed0), int(step))
  return TR.stateless_random_uniform(int(n), s0, s1) >= np.float32(rate)


def pack_bits(keep):
  """bool [n] -> uint8 [ceil(n / 8)], LSB first, spare bits 0."""
  return np.packbits(np.asarray(keep, dtype=bool), bitorder='little')


def unpack_bits(bits, n):
  return np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder='little')[:int(n)].astype(bool)


def apply_keep(x, keep, rate):
  scaled = (x.float() * torch.tensor(f32_scale(rate))).to(x.dtype)
  return torch.where(torch.from_numpy(np.asarray(keep, dtype=bool)).reshape(x.shape), scaled, torch.zeros_like(x))


def expected_fwd(x, rate, seed0, step):
  """x: CPU tensor (bf16 or fp32, any shape) -> (y, bits uint8 numpy)."""
  keep = keep_mask(x.numel(), rate, seed0, step)
  return apply_keep(x, keep, rate), pack_bits(keep)


def expected_bwd(dy, bits, rate):
  return apply_keep(dy, unpack_bits(bits, dy.numel()), rate)


def n_differing(a, b):
  """Number of elements whose bit patterns differ, NaN compared as NaN (torch's CPU casts do not keep NaN payloads)."""
  assert a.dtype == b.dtype and a.shape == b.shape
  view = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
  both_nan = torch.isnan(a) & torch.isnan(b)
  return int(((a.contiguous().view(view) != b.contiguous().view(view)) & ~both_nan).sum())
