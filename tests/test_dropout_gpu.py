"""Dropout on the GPU: rigl_dropout_fwd / _bwd / _advance bit for bit against tests/dropout_ref.py (the oracle's stateless
uniform stream + torch-CPU arithmetic) inside guard bands, on both memory paths; the autograd node; and the WideResNet with
``droprate``: unchanged at 0, fp64-twin gradients at 0.3, and fresh masks on every replay of a captured step."""
import functools

import numpy as np
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F  # noqa: E402

from tests import dropout_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD, SENTINEL = 64, 0xA5
SIZES = (1, 3, 4, 7, 8, 9, 31, 32, 2047, 2048, 2049, 65541)
RATES = (0.0, 0.3, 0.5, 0.999)
SEEDS = (-1201226755, 12345)
STEPS = (0, 1, (1 << 31) - 1)
DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}


@functools.lru_cache(maxsize=None)
def _keep(rate, seed0, step):
  """The oracle's keep mask at the largest size; element i of the stream does not depend on n, so every size is a prefix."""
  return R.keep_mask(max(SIZES), rate, seed0, step)


@functools.lru_cache(maxsize=None)
def _values(dtype_name, salt):
  gen = torch.Generator().manual_seed(100 + salt)
  return (torch.randn(max(SIZES), generator=gen) * 3).to(DTYPES[dtype_name])


def _guarded(n, dtype, offset):
  """An [n] view of ``dtype`` that starts ``offset`` elements past a 16-byte aligned address, inside SENTINEL-filled guard
  bands of GUARD bytes each side.  Returns (raw uint8 buffer, view, first payload byte)."""
  esize = torch.empty(0, dtype=dtype).element_size()
  lo = GUARD + offset * esize
  raw = torch.full((lo + n * esize + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
  return raw, raw[lo:lo + n * esize].view(dtype), lo


def _guards_intact(raw, lo, nbytes):
  return bool((raw[:lo] == SENTINEL).all()) and bool((raw[lo + nbytes:] == SENTINEL).all())


def _expect(x_cpu, keep, rate):
  return R.apply_keep(x_cpu, keep, rate), R.pack_bits(keep)


def _run_fwd(x_cpu, rate, seed0, step_t, offset):
  """rigl_dropout_fwd into guarded y / bits, from an x at the same misalignment.  Returns (y cpu, bits numpy) after checking
  the guard bands."""
  from rigl_amd import ops
  n, dtype = x_cpu.numel(), x_cpu.dtype
  _, x, _ = _guarded(n, dtype, offset)
  x.copy_(x_cpu)
  yraw, y, ylo = _guarded(n, dtype, offset)
  braw, bits, blo = _guarded((n + 7) // 8, torch.uint8, 0)
  ops.dropout_fwd(x, rate, seed0, step_t, y=y, bits=bits)
  torch.cuda.synchronize()
  assert _guards_intact(yraw, ylo, n * x.element_size()), 'y guard band overwritten'
  assert _guards_intact(braw, blo, (n + 7) // 8), 'keep_bits guard band overwritten'
  return y.cpu(), bits.cpu().numpy()


# ---- 1. forward, bit-exact, both memory paths ---------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1, 3])         # 0: 16-byte lanes + element-wise tail; 1, 3: element-wise throughout
@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_forward_is_bit_exact_inside_guard_bands(dtype_name, offset):
  step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
  for step in STEPS:
    step_t.fill_(step)
    for seed0 in SEEDS:
      for rate in RATES:
        keep_all = _keep(rate, seed0, step)
        for n in SIZES:
          x = _values(dtype_name, 0)[:n]
          want_y, want_bits = _expect(x, keep_all[:n], rate)
          y, bits = _run_fwd(x, rate, seed0, step_t, offset)
          what = (dtype_name, offset, n, rate, seed0, step)
          assert np.array_equal(bits, want_bits), what
          assert R.n_differing(y, want_y) == 0, what
          if n % 8:
            assert int(bits[-1]) >> (n % 8) == 0, what            # spare bits of the last byte
          if rate == 0.0:
            assert R.n_differing(y, x) == 0 and (bits[:n // 8] == 0xFF).all(), what
  assert int(step_t) == STEPS[-1]                                 # the forward only reads the counter


# ---- 2. special values at kept and dropped positions --------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_special_values(dtype_name, offset):
  dtype = DTYPES[dtype_name]
  n, rate, seed0, step = 64, 0.5, 12345, 4
  keep = R.keep_mask(n, rate, seed0, step)
  kept, dropped = np.flatnonzero(keep), np.flatnonzero(~keep)
  specials = [float('inf'), -float('inf'), float('nan'), -0.0, float(torch.finfo(dtype).max)]   # max * 2 overflows to inf (RNE)
  assert len(kept) >= len(specials) and len(dropped) >= len(specials)
  x = torch.ones(n, dtype=dtype)
  for j, v in enumerate(specials):
    x[int(kept[j])] = v
    x[int(dropped[j])] = v
  want_y, want_bits = _expect(x, keep, rate)
  assert torch.isinf(want_y[int(kept[4])]) and torch.isnan(want_y[int(kept[2])])
  step_t = torch.full((1,), step, dtype=torch.int32, device=DEV)
  y, bits = _run_fwd(x, rate, seed0, step_t, offset)
  assert np.array_equal(bits, want_bits)
  assert R.n_differing(y, want_y) == 0                         # NaN compared as NaN
  view = torch.int16 if dtype == torch.bfloat16 else torch.int32
  assert int(y.view(view)[torch.from_numpy(dropped)].abs().max()) == 0     # +0, bit for bit, at every dropped position
  assert int(y[int(kept[3])].view(view)) != 0                  # a kept -0 stays -0


# ---- 3. backward from the stored bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize('offset', [0, 3])
@pytest.mark.parametrize('dtype_name', ['bf16', 'fp32'])
def test_backward_is_bit_exact_from_stored_bits(dtype_name, offset):
  from rigl_amd import ops
  dtype, rate, seed0, step = DTYPES[dtype_name], 0.3, 12345, 1
  step_t = torch.zeros(1, dtype=torch.int32, device=DEV)
  for n in (1, 7, 9, 2049, 65541):
    step_t.fill_(step)
    _, x, _ = _guarded(n, dtype, offset)
    x.copy_(_values(dtype_name, 0)[:n])
    _, bits = ops.dropout_fwd(x, rate, seed0, step_t)
    ops.dropout_advance(step_t)                                # the counter moves between forward and backward
    dy_cpu = _values(dtype_name, 1)[:n]
    _, dy, _ = _guarded(n, dtype, offset)
    dy.copy_(dy_cpu)
    raw, dx, lo = _guarded(n, dtype, offset)
    ops.dropout_bwd(dy, bits, rate, dx=dx)
    torch.cuda.synchronize()
    assert _guards_intact(raw, lo, n * dx.element_size())
    want_bits = R.pack_bits(_keep(rate, seed0, step)[:n])      # the FORWARD's mask
    assert np.array_equal(bits.cpu().numpy(), want_bits)
    assert R.n_differing(dx.cpu(), R.expected_bwd(dy_cpu, want_bits, rate)) == 0, (dtype_name, offset, n)
    assert int(step_t) == step + 1


# ---- 4. the step lives on the device ------------------------------------------------------------------------------------
@pytest.mark.parametrize('step', [0, 5, (1 << 31) - 1])           # the last one wraps to -2^31 like the int32 seed pair
def test_device_resident_step(step):
  from rigl_amd import ops
  n, rate, seed0 = 2049, 0.3, -1201226755
  x_cpu = _values('bf16', 0)[:n]
  x = x_cpu.to(DEV)
  step_t = torch.full((1,), step, dtype=torch.int32, device=DEV)
  y, bits = ops.dropout_fwd(x, rate, seed0, step_t)
  first = (y.cpu(), bits.cpu().numpy())
  ops.dropout_advance(step_t)
  ops.dropout_fwd(x, rate, seed0, step_t, y=y, bits=bits)         # the same call on the same buffers
  torch.cuda.synchronize()
  nxt = step + 1 if step + 1 < (1 << 31) else -(1 << 31)
  assert int(step_t) == nxt
  for got, s in ((first, step), ((y.cpu(), bits.cpu().numpy()), nxt)):
    want_y, want_bits = R.expected_fwd(x_cpu, rate, seed0, s)
    assert np.array_equal(got[1], want_bits) and R.n_differing(got[0], want_y) == 0, s
  assert not np.array_equal(first[1], bits.cpu().numpy())


# ---- 5. the autograd node -----------------------------------------------------------------------------------------------
def test_autograd_node_saves_only_the_bits():
  from rigl_amd.workloads import nn as gnn
  n, rate, seed0 = 4 * 8 * 8 * 16, 0.3, 12345
  x_cpu = _values('bf16', 0)[:n].reshape(4, 8, 8, 16)
  x = x_cpu.to(DEV).requires_grad_(True)
  x.bn_partials = x.bn_apply = x.bn_pending = object()     # what a batch norm / conv leaves on its output
  state = gnn.DropoutState(DEV)
  state.step.fill_(2)
  y = gnn.dropout(x, rate, seed0, state)
  for attr in ('bn_partials', 'bn_apply', 'bn_pending'):
    assert not hasattr(y, attr)
  saved = y.grad_fn.saved_tensors
  assert len(saved) == 1 and saved[0].dtype == torch.uint8 and saved[0].numel() == n // 8
  assert all(t.numel() != n for t in saved)
  want_y, want_bits = R.expected_fwd(x_cpu, rate, seed0, 2)
  assert R.n_differing(y.detach().cpu(), want_y) == 0
  dy_cpu = _values('bf16', 1)[:n].reshape(x_cpu.shape)
  state.step.fill_(9)                                             # the backward must not look at the counter
  y.backward(dy_cpu.to(DEV))
  assert R.n_differing(x.grad.cpu(), R.expected_bwd(dy_cpu, want_bits, rate)) == 0
  assert gnn.dropout(x, rate, seed0, state, is_training=False) is x and gnn.dropout(x, 0.0, seed0, state) is x


# ---- 6. the model is unchanged at droprate 0 ----------------------------------------------------------------------------
def _model_outputs(**kw):
  from rigl_amd import train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=10, width=1, seed=0, **kw)
  x, y = wide_resnet.synthetic_batch(8, DEV)
  out = dict(model=model)
  with torch.no_grad():
    out['eval'] = model(x, is_training=False).float().cpu()
  out['infer'] = model.infer(x).cpu()
  losses = []
  for _ in range(2):
    loss = model.loss(x, y)
    train.MomentumOptimizer(0.1, 0.9, graph=g).compute_gradients(loss)
    losses.append(float(loss.detach()))
  torch.cuda.synchronize()
  out['losses'], out['G'] = losses, g.G.detach().cpu().clone()
  return out


def test_model_is_unchanged_at_droprate_zero():
  a, b, c = _model_outputs(), _model_outputs(droprate=0.0), _model_outputs(droprate=0.3)
  assert a['model'].dropout_state is None and b['model'].dropout_state is None
  assert a['losses'] == b['losses'] and a['losses'][0] == a['losses'][1]
  assert torch.equal(a['G'].view(torch.int32), b['G'].view(torch.int32))
  assert torch.equal(a['infer'].view(torch.int32), b['infer'].view(torch.int32))
  # eval paths of the dropout model: nothing new
  assert torch.equal(a['infer'].view(torch.int32), c['infer'].view(torch.int32))
  assert torch.equal(a['eval'].view(torch.int32), c['eval'].view(torch.int32))
  # training: two forwards, two different masks
  assert c['losses'][0] != c['losses'][1] and c['losses'][0] != a['losses'][0]
  assert int(c['model'].dropout_state.step) == 2


# ---- 7. gradients of the model with dropout against an fp64 twin --------------------------------------------------------
class _RoundBF16(torch.autograd.Function):
  """bf16 rounding of a tensor in the forward AND of its gradient in the backward pass (tests/test_network_grad_gpu.py), fp64."""

  @staticmethod
  def forward(ctx, x):
    return x.to(torch.bfloat16).double()

  @staticmethod
  def backward(ctx, g):
    return g.to(torch.bfloat16).double()


def _twin(model, x_nhwc, labels, keeps, rounding):
  """The network of tests/test_network_grad_gpu.py::_reference in fp64 on the CPU, with the keep masks and 1 / (1 - rate)
  applied after bn_b's ReLU.  Returns (loss, {scope: dL/d(mask * W) in HWIO})."""
  rnd = _RoundBF16.apply if rounding else (lambda t: t)
  leaves = {}
  scale = float(R.f32_scale(model.droprate))

  def weights(layer):
    w = layer.weights.data.detach().cpu().double()
    if layer.mask is not None:
      w = w * layer.mask.data.detach().cpu().double().reshape(w.shape)
    if rounding:
      w = w.to(torch.bfloat16).double()
    w = w.clone().requires_grad_(True)
    leaves[layer.scope] = w
    return w

  def conv(layer, x, k, stride):
    w = weights(layer).permute(3, 2, 0, 1)
    if k == 3:                                              # TF 'SAME': the extra pixel at the end
      h, wd = x.shape[2], x.shape[3]
      th = max((-(-h // stride) - 1) * stride + 3 - h, 0)
      tw = max((-(-wd // stride) - 1) * stride + 3 - wd, 0)
      x = F.pad(x, (tw // 2, tw - tw // 2, th // 2, th - th // 2))
    return rnd(F.conv2d(x, w, stride=stride))

  def bn_relu(bn, x):
    y = F.batch_norm(x, None, None, bn.gamma.data.cpu().double(), bn.beta.data.cpu().double(), True, 0.1, bn.eps)
    return rnd(F.relu(y))

  net = conv(model.stem, x_nhwc.cpu().double().permute(0, 3, 1, 2), 3, 1)
  for i, b in enumerate(model.blocks):
    skip = net
    net = bn_relu(b['bn_a'], net)
    if 'skip' in b:
      skip = conv(b['skip'], net, 1, b['skip'].strides[0])
    net = conv(b['conv1'], net, 3, b['conv1'].strides[0])
    net = bn_relu(b['bn_b'], net)
    net = rnd(net * keeps[i] * scale)
    net = conv(b['conv2'], net, 3, 1)
    net = rnd(net + skip)
  net = bn_relu(model.final_bn, net)
  feat = rnd(net.mean(dim=(2, 3)))
  logits = rnd(feat @ weights(model.logits) + model.logits.bias.data.cpu().double())
  loss = F.cross_entropy(logits, labels.cpu())
  loss.backward()
  return float(loss.detach()), {k: v.grad for k, v in leaves.items()}


def test_model_gradients_with_dropout_vs_fp64_twin():
  """The method and the tolerances of tests/test_network_grad_gpu.py (per layer: relative L2 <= 0.15, cosine >= 0.99 and norm
  within 5 % against the rounding-point reference; 0.35 / 0.95 against plain arithmetic; loss within 1e-4), on depth 10 at
  batch 8 with droprate 0.3.  The twin applies the masks the kernels stored."""
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=10, width=1, droprate=0.3, dropout_seed=11)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  gen = torch.Generator(device=DEV).manual_seed(3)
  for mod in g.modules.values():
    if hasattr(mod, 'gamma'):
      mod.gamma.data.copy_(1.0 + 0.2 * torch.randn(mod.channels, generator=gen, device=DEV))
      mod.beta.data.copy_(0.1 * torch.randn(mod.channels, generator=gen, device=DEV))
  inner = train.MomentumOptimizer(0.1, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 75000, 100, drop_fraction=0.3, noise_std=0.)
  x, y = wide_resnet.synthetic_batch(8, DEV)
  stored = {}
  model.dropout_state.bits_hook = lambda seed0, bits: stored.__setitem__(seed0, bits.clone())
  loss = model.loss(x, y)
  opt.compute_gradients(loss)
  torch.cuda.synchronize()
  assert int(model.dropout_state.step) == 1 and len(stored) == len(model.blocks) == 3
  keeps = []
  for i, b in enumerate(model.blocks):
    cout = b['conv1'].weights.shape[-1]
    hw = 32 // (1, 2, 4)[i]
    n = 8 * hw * hw * cout
    bits = stored[model.dropout_seed0(i)].cpu().numpy()
    assert np.array_equal(bits, R.pack_bits(R.keep_mask(n, 0.3, model.dropout_seed0(i), 1)))    # the mask the oracle draws
    keeps.append(torch.from_numpy(R.unpack_bits(bits, n)).reshape(8, hw, hw, cout).permute(0, 3, 1, 2).double())
  mine = {l.scope: l.weights.grad.detach().cpu().double().reshape(l.weights.shape).clone() for l in g.layers}
  figures = {}
  for rounding, tol_rel, tol_cos, tol_loss in ((True, 0.15, 0.99, 1e-4), (False, 0.35, 0.95, 1e-4)):
    ref_loss, ref = _twin(model, x, y, keeps, rounding)
    rows = {}
    for scope, dw in mine.items():
      r = ref[scope].reshape(dw.shape)
      rows[scope] = (float((dw - r).norm() / r.norm()), float((dw * r).sum() / (dw.norm() * r.norm())), float(dw.norm() / r.norm()))
    figures[rounding] = (float(loss.detach()), ref_loss, rows)
    print('rounding=%s loss %.6f ref %.6f worst rel %.4f worst cos %.4f' % (
        rounding, float(loss.detach()), ref_loss, max(v[0] for v in rows.values()), min(v[1] for v in rows.values())))
    assert abs(float(loss.detach()) - ref_loss) <= tol_loss * abs(ref_loss), figures[rounding][:2]
    for scope, (rel, cos, ratio) in rows.items():
      assert rel <= tol_rel and cos >= tol_cos, (rounding, scope, rel, cos)
      if rounding:
        assert 0.95 <= ratio <= 1.05, (scope, ratio)


# ---- 8. graph replay ----------------------------------------------------------------------------------------------------
def _run(graphed, steps):
  """tests/test_graphed_step_gpu.py::_run with droprate 0.3; block 0's keep bits are copied out after every forward."""
  from rigl_amd import sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=10, width=1, droprate=0.3)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  inner = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.)
  gs = g.get_or_create_global_step()
  x, y = wide_resnet.synthetic_batch(32, DEV)
  seed_b0, n_b0 = model.dropout_seed0(0), 32 * 32 * 32 * 16
  bits_b0 = torch.zeros(n_b0 // 8, dtype=torch.uint8, device=DEV)         # allocated before any capture: outlives the graph's pool

  def hook(seed0, bits):
    if seed0 == seed_b0:
      bits_b0.copy_(bits)                                                   # captured with the step, so replayed with it
  model.dropout_state.bits_hook = hook
  loss_fn = lambda: model.loss(x, y)
  if graphed:
    st = train.GraphedStep(loss_fn, opt, gs, warmup=2)
    run = st
  else:
    st = None

    def run():
      loss = loss_fn()
      opt.minimize(loss, gs)
      return loss
  losses, seen = [], []
  for _ in range(steps):
    before = st.replays if st is not None else 0
    losses.append(float(run().detach().float()))
    seen.append((st is not None and st.replays > before, int(model.dropout_state.step), bits_b0.cpu().numpy().copy()))
  torch.cuda.synchronize()
  out = dict(W=g.W.cpu().numpy().copy(), A=inner._slot.cpu().numpy().copy(), B=g.BITS.cpu().numpy().copy(),
             gs=int(gs.value), losses=losses, step=int(model.dropout_state.step), seen=seen, seed_b0=seed_b0, n_b0=n_b0)
  if st is not None:
    out['replays'], out['eager'] = st.replays, st.eager_steps
  return out


def test_graph_replay_draws_fresh_masks_and_matches_eager():
  steps = 19
  a = _run(False, steps)
  b = _run(True, steps)
  assert b['replays'] >= 8 and b['eager'] >= 4
  assert a['gs'] == b['gs'] == steps - 4
  np.testing.assert_array_equal(a['B'], b['B'])
  np.testing.assert_array_equal(a['W'].view(np.uint32), b['W'].view(np.uint32))
  np.testing.assert_array_equal(a['A'].view(np.uint32), b['A'].view(np.uint32))
  assert a['losses'] == b['losses']
  # one executed training forward per call -- eager, warm-up or replay; the capture pass itself enqueues nothing
  assert a['step'] == b['step'] == steps
  assert [s[1] for s in b['seen']] == list(range(1, steps + 1))
  # two consecutive replays: different keep bits, each the oracle's mask at the counter that replay read
  pairs = [i for i in range(1, steps) if b['seen'][i][0] and b['seen'][i - 1][0]]
  assert pairs
  i = pairs[0]
  (_, s0, bits0), (_, s1, bits1) = b['seen'][i - 1], b['seen'][i]
  assert s1 == s0 + 1 and not np.array_equal(bits0, bits1)
  for s, bits in ((s0, bits0), (s1, bits1)):
    assert np.array_equal(bits, R.pack_bits(R.keep_mask(b['n_b0'], 0.3, b['seed_b0'], s)))
