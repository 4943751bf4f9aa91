"""bench.py's contract pieces that do not need a GPU: the flag defaults the driver relies on, the committed PMC summary the
``roofline.traffic`` field is read from, and the loud failure when no MI355X is visible (there is no CPU fallback to time)."""
import importlib.util
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location('vited_bench', os.path.join(ROOT, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_defaults(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py'])
    a = bench.parse()
    assert a.gpus == 1 and a.steps >= 1 and a.warmup >= 0 and a.workload == 'A-train'
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--gpus', '8', '--steps', '7', '--warmup', '3'])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (8, 7, 3)
    assert a.dump_outputs is None
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--dump-outputs', 'out'])
    assert bench.parse().dump_outputs == 'out'


def test_steps_below_one_are_refused(monkeypatch):
    import pytest
    bench = _bench()
    monkeypatch.setattr(sys, 'argv', ['bench.py', '--steps', '0'])
    with pytest.raises(SystemExit):
        bench.parse()


def test_dump_outputs_dtypes_budget_and_fixed_sample(tmp_path):
    import numpy as np
    import torch
    bench = _bench()
    g = torch.Generator().manual_seed(1)
    arrays = {'loss': torch.tensor(0.5, dtype=torch.float64), 'small': torch.randn(3, 4, generator=g),
              'half': torch.randn(100, generator=g).to(torch.bfloat16), 'big': torch.randn(1000, 50, generator=g)}
    budget = 4096
    bench.dump_outputs(str(tmp_path / 'a'), arrays, budget=budget)
    bench.dump_outputs(str(tmp_path / 'b'), arrays, budget=budget)
    got = {n: np.load(tmp_path / 'a' / f'{n}.npy') for n in arrays}
    assert got['loss'].dtype == np.float64 and float(got['loss']) == 0.5
    assert all(got[n].dtype == np.float32 for n in ('small', 'half', 'big'))
    assert np.array_equal(got['small'], arrays['small'].numpy())                       # fits: whole, shape kept
    assert np.array_equal(got['half'], arrays['half'].float().numpy())
    assert sum(a.nbytes for a in got.values()) <= budget and 0 < got['big'].size < 50000
    assert np.all(np.isin(got['big'], arrays['big'].numpy()))                          # a sample of the real elements
    for n in arrays:                                                                   # the same sample in every run
        assert np.array_equal(got[n], np.load(tmp_path / 'b' / f'{n}.npy'))


def test_committed_pmc_summary_covers_the_dominant_kernel_classes():
    bench = _bench()
    for cls in ('gemm_nt_mfma_kernel', 'gemm_tn_wide_kernel', 'gemm_row_kernel'):
        t = bench.pmc_traffic(cls)
        assert t['traffic'] and t['traffic'] > 1e6, cls          # bytes per launch
    assert bench.pmc_traffic('no_such_kernel') == {'traffic': None}
    assert bench.PEAK_BF16_DENSE_TFLOPS == 2500.0 and bench.PEAK_HBM_GBPS == 8000.0   # MI355X_MICROARCH.md sheet values


def test_refuses_to_run_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        import pytest
        pytest.skip('a GPU is visible')
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--steps', '1', '--warmup', '0'], capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode != 0
    assert 'no GPU is visible' in (r.stderr + r.stdout)
    assert '"metric"' not in r.stdout           # no JSON line from a machine that did not measure
