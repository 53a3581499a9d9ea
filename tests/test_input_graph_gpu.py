"""The device input pipeline under graph replay: a captured ``DeviceCifar.next_batch()`` produces the reference's batch for
every replayed step, across an epoch boundary; and a WideResNet trained from it under train.GraphedStep leaves the losses of
the same steps run eagerly."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

from tests import input_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def test_captured_next_batch_replays_fresh_batches_across_an_epoch_boundary():
  from rigl_amd import data
  n, batch = 37, 8
  images, labels = R.dataset(n)
  dc = data.DeviceCifar(images, labels, batch, seed=R.TRAIN_SEED, device=DEV, with_indices=True)
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    dc.next_batch()                                              # code objects load outside the capture
  torch.cuda.current_stream().wait_stream(side)
  torch.cuda.synchronize()
  dc.seek(0)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    x, y = dc.next_batch()
  assert dc.position() == 0                                      # a capture enqueues nothing
  for step in range(6):                                          # 4 steps per epoch: replay 4 is the first of epoch 1
    graph.replay()
    torch.cuda.synchronize()
    want = R.batch(images, labels, batch, step, R.BF16, seed0=R.TRAIN_SEED)
    assert np.array_equal(R.tensor_bits(x), want[0]), step
    assert np.array_equal(y.cpu().numpy(), want[1]), step
    assert np.array_equal(dc.last_indices().cpu().numpy(), want[2]), step
    assert dc.position() == step + 1
  # a frozen epoch would repeat step 0's images at step 4: the reference's two orders differ
  assert not np.array_equal(R.train_indices(n, batch, R.TRAIN_SEED, 4), R.train_indices(n, batch, R.TRAIN_SEED, 0))


def _run(graphed, steps):
  """tests/test_graphed_step_gpu.py::_run on the smallest WideResNet, fed by a DeviceCifar inside loss_fn."""
  from rigl_amd import data, sparse_optimizers as SO, sparse_utils, train, variables as V
  from rigl_amd.workloads import wide_resnet
  g = V.reset_default_graph(DEV)
  model = wide_resnet.WideResNet(g, depth=10, width=1)
  np.random.seed(0)
  sparse_utils.get_mask_init_fn(g.get_masks(), 'erdos_renyi_kernel', 0.8, {})()
  inner = train.MomentumOptimizer(0.05, 0.9, use_nesterov=True, graph=g)
  opt = SO.SparseRigLOptimizer(inner, 0, 1000, 5, drop_fraction=0.3, drop_fraction_anneal='cosine', noise_std=0.)
  gs = g.get_or_create_global_step()
  images, labels = R.dataset(64, plant=False)
  dc = data.DeviceCifar(images, labels, 16, seed=5, device=DEV, with_indices=True)

  def loss_fn():
    x, y = dc.next_batch()
    return model.loss(x, y)
  if graphed:
    st = train.GraphedStep(loss_fn, opt, gs, warmup=1)
    run = st
  else:
    st = None

    def run():
      loss = loss_fn()
      opt.minimize(loss, gs)
      return loss
  losses, indices = [], []
  for _ in range(steps):
    losses.append(float(run().detach().float()))
    indices.append(dc.last_indices().cpu().numpy().copy())
  torch.cuda.synchronize()
  out = dict(losses=losses, indices=indices, position=dc.position(), gs=int(gs.value))
  if st is not None:
    out['replays'], out['eager'] = st.replays, st.eager_steps
  return out


def test_graphed_wide_resnet_trains_on_the_same_batches_as_eager():
  steps = 11                        # calls 0 and 6 are mask updates (eager); 4 steps per epoch: two epoch boundaries
  a = _run(False, steps)
  b = _run(True, steps)
  assert b['replays'] > 0 and b['eager'] > 0 and b['replays'] + b['eager'] == steps
  assert a['position'] == b['position'] == steps
  assert a['gs'] == b['gs']
  for s in range(steps):
    assert np.array_equal(a['indices'][s], R.train_indices(64, 16, 5, s)), s
    assert np.array_equal(b['indices'][s], a['indices'][s]), s
  assert a['losses'] == b['losses']
  assert len(set(a['losses'])) == steps                           # fresh data every step: no two losses alike
