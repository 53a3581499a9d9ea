"""NumPy fp32 restatement of gradual magnitude pruning as TF 1.15's
contrib/model_pruning/python/pruning.py computes it (Pruning._setup_sparsity,
_get_sparsity, conditional_mask_update_op, _update_mask; weight magnitude, 1x1
blocks) -- the yardstick of tests/test_pruning_*.py.  Documented, not executed:
contrib is not available offline, so these rules are the spec.  Every fp32
operation is rounded separately.  Written independently of rigl_amd.pruning."""
import numpy as np

F32 = np.float32


def sparsity(step, initial=0.0, target=0.5, begin=0, end=100, exponent=3):
  """p = min(1, max(0, f32(t - b) / f32(e - b))); s = f32(initial - target) * powf(1 - p, f32(exponent)) + target."""
  with np.errstate(divide='ignore', invalid='ignore'):
    p = F32(min(F32(1), max(F32(0), F32(F32(step - begin) / F32(end - begin)))))
  return F32(F32(F32(initial - target) * F32(np.power(F32(F32(1) - p), F32(exponent)))) + F32(target))


def layer_sparsity(weight_name, s, sparsity_map, target=0.5):
  """A map entry matches when its name is a substring of the weight op name; s * (value / target) in fp32."""
  hits = [v for k, v in sparsity_map.items() if weight_name.find(k) != -1]
  if len(hits) > 1:
    raise ValueError('Multiple matches in weight_sparsity_map for weight %s' % weight_name)
  if not hits:
    return F32(s)
  return F32(F32(s) * F32(F32(hits[0]) / F32(target)))


def gate(step, last_update, begin=0, end=-1, frequency=10):
  """conditional_mask_update_op's predicate."""
  in_range = step >= begin and (step <= end or end < 0)
  return bool(in_range and last_update + frequency <= step)


def k_of(n, s_l):
  """k = round_half_even(f32(n) * (1 - s_l)) (tf.round is banker's rounding)."""
  return int(np.rint(F32(F32(n) * F32(F32(1) - F32(s_l)))))


def mask_update(w, k, threshold=0.0, decay=0.0):
  """One _update_mask on the raw weights: returns (new threshold (fp32), mask (uint8 0/1, w's shape))."""
  if k == 0:
    raise ValueError('k == 0: gather(values, -1)')
  a = np.abs(np.asarray(w, F32)).reshape(-1)
  values = np.sort(a, kind='stable')[::-1]          # top_k(|W|, size) values, descending
  cur = F32(values[k - 1])
  thr = F32(F32(cur * F32(1.0 - decay)) + F32(F32(threshold) * F32(decay)))
  mask = (np.abs(np.asarray(w, F32)) >= thr).astype(np.uint8)
  return thr, mask


def pack_bits(mask01):
  """0/1 array -> uint32 bitmap words, flat C order, bit i of word j = element 32j + i, tail bits zero."""
  m = np.asarray(mask01).reshape(-1).astype(np.uint8)
  pad = (-m.size) % 32
  m = np.concatenate([m, np.zeros(pad, np.uint8)])
  return np.packbits(m, bitorder='little').view('<u4').astype(np.uint32)
