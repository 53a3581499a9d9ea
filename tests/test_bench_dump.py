"""bench.py --dump-outputs: the host side of the snapshot (sampling, mask bit order, sizes) on stand-in arenas, and the
--steps guard.  Run in a child process: importing bench.py sets environment defaults for the HSA runtime."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = r'''
import json, os, sys, tempfile, types
import numpy as np, torch
sys.path.insert(0, sys.argv[1])
import bench
from rigl_amd import variables
res = []
for n_masked, total in ((96, 160), (5000000, 5200000)):
  rs = np.random.RandomState(3)
  m = (rs.rand(n_masked) < 0.2).astype(np.float32)
  words = np.packbits(m.astype(np.uint8), bitorder='little').view(np.int32)
  g = types.SimpleNamespace(W=torch.randn(total), G=torch.randn(total), BITS=torch.from_numpy(words.copy()),
                            seg={variables.KIND_MASKED: (0, n_masked)})
  inner = types.SimpleNamespace(_slot=torch.randn(total))
  out = bench.snapshot_outputs(g, inner, torch.tensor(2.5, dtype=torch.bfloat16))
  again = bench.snapshot_outputs(g, inner, torch.tensor(2.5, dtype=torch.bfloat16))
  d = tempfile.mkdtemp()
  bench.write_outputs(os.path.join(d, 'o'), out)
  files = sorted(os.listdir(os.path.join(d, 'o')))
  back = {f[:-4]: np.load(os.path.join(d, 'o', f)) for f in files}
  res.append(dict(
      files=files, dtypes=sorted({str(a.dtype) for a in back.values()}),
      nbytes=int(sum(a.nbytes for a in back.values())),
      mask_ok=bool(np.array_equal(back['mask'], bench._dump_sample(m))),
      weights_ok=bool(np.array_equal(back['weights'], bench._dump_sample(g.W.numpy()))),
      momentum_ok=bool(np.array_equal(back['momentum'], bench._dump_sample(inner._slot.numpy()))),
      repeatable=all(np.array_equal(out[k], again[k]) for k in out),
      loss=float(back['loss'][0]), n=[int(a.size) for a in (back['weights'], back['mask'])]))
print(json.dumps(res))
'''


def test_dump_outputs_snapshot_on_host_arenas():
  r = subprocess.run([sys.executable, '-c', _CHILD, ROOT], capture_output=True, text=True, timeout=300)
  assert r.returncode == 0, r.stderr[-2000:]
  small, large = json.loads(r.stdout.strip().splitlines()[-1])
  for c in (small, large):
    assert c['files'] == ['grad.npy', 'loss.npy', 'mask.npy', 'momentum.npy', 'weights.npy']
    assert c['dtypes'] == ['float32']
    assert c['mask_ok'] and c['weights_ok'] and c['momentum_ok'] and c['repeatable']
    assert c['loss'] == 2.5
    assert c['nbytes'] <= 64 << 20
  assert small['n'] == [160, 96]                       # small arenas are written whole
  assert large['n'] == [1 << 21, 1 << 21]              # large ones as the fixed sample


def test_bench_refuses_zero_steps():
  r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '0'],
                     capture_output=True, text=True, timeout=300)
  assert r.returncode == 2 and '--steps must be at least 1' in r.stderr
