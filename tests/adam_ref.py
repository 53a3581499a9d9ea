"""NumPy fp32 restatement of TF's ApplyAdam (training_ops.cc, non-Nesterov) with
the masked gradient of K3 -- the yardstick of tests/test_adam_*.py.  Every
product and sum is rounded to fp32 separately; sqrt and division are the
correctly rounded fp32 operations."""
import numpy as np

from oracle import rigl_oracle as O

F32 = np.float32


def alpha(lr, beta_powers):
  """(lr * sqrt(1 - beta2_power)) / (1 - beta1_power)."""
  b1p, b2p = F32(beta_powers[0]), F32(beta_powers[1])
  return F32(F32(F32(lr) * F32(np.sqrt(F32(F32(1) - b2p)))) / F32(F32(1) - b1p))


def masked_grad(dense, mask, w, weight_decay=0.0, grad_scale=1.0):
  """g = mask * (grad_scale*dense) + wd*w: oracle.masked_grad (the reference's own form, zero signs included) on the
  scaled gradient; mask None = all ones.  For finite inputs rigl_masked_sgd_momentum forms the same bits, and
  rigl_masked_adam the same up to the sign of a zero, which none of its results depends on."""
  dense = np.asarray(dense, F32)
  gs = dense if F32(grad_scale) == F32(1) else (dense * F32(grad_scale)).astype(F32)
  m = np.ones_like(gs) if mask is None else (np.asarray(mask) != 0).astype(F32)
  return O.masked_grad(gs, m, w, weight_decay)


def adam_apply(w, m, v, g, lr, beta_powers, beta1=0.9, beta2=0.999, epsilon=1e-8):
  """One ApplyAdam on fp32 arrays; returns (w, m, v)."""
  a = alpha(lr, beta_powers)
  omb1 = F32(F32(1) - F32(beta1))
  omb2 = F32(F32(1) - F32(beta2))
  g = np.asarray(g, F32)
  m = (m + ((g - m).astype(F32) * omb1).astype(F32)).astype(F32)
  v = (v + (((g * g).astype(F32) - v).astype(F32) * omb2).astype(F32)).astype(F32)
  den = (np.sqrt(v).astype(F32) + F32(epsilon)).astype(F32)
  w = (w - ((m * a).astype(F32) / den).astype(F32)).astype(F32)
  return w, m, v


def advance(beta_powers, beta1=0.9, beta2=0.999):
  """AdamOptimizer._finish: one fp32 product per accumulator."""
  return np.array([F32(F32(beta_powers[0]) * F32(beta1)), F32(F32(beta_powers[1]) * F32(beta2))], F32)


def same_bits(a, b):
  """Bit-identical, except that NaNs compare as NaNs (their payloads differ between x86 and gfx950)."""
  a = np.asarray(a, F32).reshape(-1)
  b = np.asarray(b, F32).reshape(-1)
  na, nb = np.isnan(a), np.isnan(b)
  return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint32), b[~nb].view(np.uint32)))
