"""bench.py --gpus N: the N-rank launch is decided before anything touches a GPU, runs as a child
torchrun job (never an exec), and fails cleanly when fewer GPUs are visible (this CPU container)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _forbid_gpu_init(monkeypatch):
    """The launcher must not initialise the GPU.  torch.cuda.is_initialized() shows that only while
    nothing earlier in this process has used the GPU (a test module that sorts before this one may
    have), so any initialisation attempt made meanwhile fails too.  Returns the state before."""
    def boom(*a, **k):
        raise AssertionError('launcher initialised the GPU')
    monkeypatch.setattr(torch.cuda, '_lazy_init', boom)
    monkeypatch.setattr(torch.cuda, 'init', boom)
    return torch.cuda.is_initialized()


def test_launch_plan_is_pure_and_device_free(monkeypatch):
    import bench
    was = _forbid_gpu_init(monkeypatch)
    cmd = bench.launch_plan(4, ['--gpus', '4', '--steps', '5'], {})
    assert cmd[:3] == [sys.executable, '-m', 'torch.distributed.run']
    assert '--nproc-per-node' in cmd and cmd[cmd.index('--nproc-per-node') + 1] == '4'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-3:] == ['--gpus', '4', '--steps', '5'][-3:]
    assert os.path.samefile(cmd[cmd.index('--master-port') + 2], os.path.join(ROOT, 'bench.py'))
    # already a torchrun rank, or a single GPU: this process is the job
    assert bench.launch_plan(4, [], {'WORLD_SIZE': '4'}) is None
    assert bench.launch_plan(1, [], {}) is None
    assert torch.cuda.is_initialized() == was


def test_gpus_2_without_gpus_fails_cleanly():
    env = dict(os.environ)
    env.pop('WORLD_SIZE', None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '2', '--no-cpu'],
                       capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2, (r.returncode, r.stdout[-500:], r.stderr[-2000:])
    assert 'GPU(s) visible' in r.stderr
    assert r.stdout.strip() == ''


def test_lines_beside_the_headline_need_full(capsys):
    import bench
    a = bench.parse(['--gpus', '1', '--steps', '7', '--warmup', '2'])
    assert not a.full and a.dump_outputs is None and a.steps == 7
    # off by default, also when the headline alone is named; a line beside it named with --only is
    # asked for explicitly and turns --full on
    assert not bench.parse(['--only', 'train']).full
    assert not bench.parse(['--no-cpu', '--no-infer']).full
    assert bench.parse(['--full', '--only', 'infer,p1']).full
    assert bench.parse(['--only', 'train,infer']).full and bench.parse(['--only', 'p1', '--no-cpu']).full
    assert bench.parse(['--full', '--dump-outputs', 'd']).dump_outputs == 'd'
    # the dump is of the headline step: asking for it while leaving that step out is an error
    assert bench.parse(['--full', '--only', 'train,infer', '--dump-outputs', 'd']).dump_outputs == 'd'
    with pytest.raises(SystemExit) as e:
        bench.parse(['--full', '--only', 'infer', '--dump-outputs', 'd'])
    assert e.value.code == 2 and '--dump-outputs' in capsys.readouterr().err


def _kfd(tmp_path, kinds):
    for i, simd in enumerate(kinds):
        d = tmp_path / str(i)
        d.mkdir()
        (d / 'properties').write_text('cpu_cores_count 0\nsimd_count %d\nlds_size_in_kb 160\n' % simd)
    return str(tmp_path)


def test_visible_gpus_counts_without_hip(tmp_path, monkeypatch):
    """the launcher counts GPUs from KFD sysfs / the visible-devices env; torch's device
    count (which can initialise HIP in the parent) is never called."""
    import bench
    was = _forbid_gpu_init(monkeypatch)

    def boom(*a, **k):
        raise AssertionError('launcher touched the HIP runtime')
    monkeypatch.setattr(torch.cuda, 'device_count', boom)
    monkeypatch.setattr(torch.cuda, 'is_available', boom)
    kfd = _kfd(tmp_path, [0, 1024, 1024, 1024, 1024, 1024, 1024, 1024, 1024])  # 1 CPU + 8 GPU nodes
    assert bench.visible_gpus({}, kfd) == 8
    assert bench.visible_gpus({'HIP_VISIBLE_DEVICES': '0,1'}, kfd) == 2
    assert bench.visible_gpus({'ROCR_VISIBLE_DEVICES': '3', 'HIP_VISIBLE_DEVICES': '0,1'}, kfd) == 1
    assert bench.visible_gpus({'CUDA_VISIBLE_DEVICES': ''}, kfd) == 0
    assert bench.visible_gpus({}, str(tmp_path / 'absent')) == 0
    monkeypatch.setattr(bench, 'KFD_NODES', kfd)
    calls = []
    monkeypatch.setattr(bench.subprocess, 'call', lambda cmd, env=None: calls.append(cmd) or 0)
    monkeypatch.delenv('HIP_VISIBLE_DEVICES', raising=False)
    monkeypatch.delenv('ROCR_VISIBLE_DEVICES', raising=False)
    monkeypatch.delenv('CUDA_VISIBLE_DEVICES', raising=False)
    monkeypatch.setattr(bench, 'visible_gpus', lambda env=None, kfd=kfd: 8)
    assert bench.spawn_ranks(8, ['--gpus', '8']) == 0
    assert calls and calls[0][2] == 'torch.distributed.run'
    assert torch.cuda.is_initialized() == was


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_repeatable_outputs(tmp_path, capsys):
    """A plain run times the headline steps only (no other line, no CPU baseline) and
    --dump-outputs writes the last step's arrays; the same arguments give the same arrays."""
    import json
    import numpy as np
    import bench
    lines = []
    for d in ('a', 'b'):
        bench.main(['--gpus', '1', '--steps', '2', '--warmup', '1', '--dump-outputs', str(tmp_path / d)])
        lines.append(json.loads(capsys.readouterr().out.strip().splitlines()[-1]))
    line = lines[0]
    assert line['steps'] == 2 and line['ms_per_step'] > 0 and line['unit'] == 'images/sec'
    assert line['value'] == pytest.approx(bench.PER_GPU / (line['ms_per_step'] * 1e-3))
    assert line['higher_is_better'] is True and line['dtype'] == 'fp32' and line['metric'] == bench.METRIC
    assert not {'strong', 'p1', 'infer', 'train88', 'attn', 'blazeface', 'blazeface_b1', 'cpu_baseline'} & set(line)
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['adam_m.npy', 'adam_v.npy', 'grad.npy', 'loss.npy', 'params.npy']
    total = 0
    for n in names:
        x, y = np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)
        assert x.dtype in (np.float32, np.float64) and np.isfinite(x).all(), n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += x.nbytes
    assert total <= 64 << 20
    assert float(np.load(tmp_path / 'a' / 'loss.npy')[0]) == line['train_mse_last_step']
    assert np.abs(np.load(tmp_path / 'a' / 'params.npy')).max() > 0
    # --steps sets the number of timed steps: warm-up and timed steps are the same update on the
    # same batch (dropout 0), so 2 + 1 leaves the weights and Adam moments of 1 + 2, bit for bit,
    # and 1 + 1 is one update short of them
    for d, w, s in (('c', 2, 1), ('d', 1, 1)):
        bench.main(['--gpus', '1', '--steps', str(s), '--warmup', str(w), '--dump-outputs', str(tmp_path / d)])
        capsys.readouterr()
    for n in ('params.npy', 'adam_m.npy', 'adam_v.npy'):
        a3 = np.load(tmp_path / 'a' / n)
        np.testing.assert_array_equal(a3, np.load(tmp_path / 'c' / n), err_msg=n)
        assert not np.array_equal(a3, np.load(tmp_path / 'd' / n)), n
