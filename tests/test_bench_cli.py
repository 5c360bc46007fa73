"""bench.py's command line: a plain run (the headline figure alone), --full (everything
else the line carries) and --dump-outputs (the last timed step's outputs as .npy).
The CPU tests drive bench.main in-process on one rank with the oracle stand-in of
tests/test_multiproc_cpu.py in place of the HIP op; the GPU test runs the real op."""
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONTRACT = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("roofline", "stages_ms", "e2e", "cpu_baseline", "parity", "secondary")


def _stub_run(c, images, steps, warmup, device, world, prof=None, breakdown=True):
    from test_multiproc_cpu import _stub_run as stub
    el, stages, roof, e2e, out, idx = stub(c, images, steps, warmup, device, world, prof)
    return (el, stages, roof, e2e, out, idx) if breakdown else (el, None, None, None, out, idx)


@pytest.fixture
def cpu_bench(monkeypatch):
    """bench on one CPU rank: DeiT-base shape, 3 images of 2 heads."""
    import bench
    monkeypatch.setenv("MXA_BENCH_BACKEND", "gloo")
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setitem(bench.CONFIGS, "deit_base", dict(bench.CONFIGS["deit_base"], B=3, H=2))
    return bench


def test_plain_run_prints_the_contract_line_and_nothing_that_takes_a_run_of_its_own(cpu_bench, capsys):
    res = cpu_bench.main(["--gpus", "1", "--steps", "3", "--warmup", "1"], run=_stub_run)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line == json.loads(json.dumps(res))
    assert all(k in line for k in CONTRACT) and not any(k in line for k in FULL_ONLY)
    assert line["metric"] == cpu_bench.METRIC and line["unit"] == "tokens/s" and line["dtype"] == "int8"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
    assert line["value"] == pytest.approx(3 * 197 * 3 / (line["ms_per_step"] * 3 / 1e3))
    assert cpu_bench.DUMP_BYTES <= 64 << 20


def test_full_run_keeps_every_block_of_the_line(cpu_bench):
    res = cpu_bench.main(["--full", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-secondary", "--no-cpu-baseline"],
                         run=_stub_run)
    assert all(k in res for k in CONTRACT + ("roofline", "stages_ms", "e2e", "cpu_baseline", "parity"))
    assert res["parity"]["idx_bitmatch"] == 1.0 and res["parity"]["images_checked"] == 2
    order = list(res)  # the line's layout is what it was before --full existed
    assert order.index("config") < order.index("roofline") < order.index("cpu_baseline") < order.index("dist")


@pytest.mark.parametrize("opt", [["--lines", "main"], ["--traffic-json", "t.json"], ["--pmc-json", "p.json"]])
def test_options_of_the_full_run_are_refused_without_it(cpu_bench, opt):
    with pytest.raises(SystemExit, match="need --full"):
        cpu_bench.main(["--steps", "1"] + opt, run=_stub_run)


def test_dump_outputs_writes_the_outputs_as_float_arrays(cpu_bench, tmp_path):
    from oracle import mx_oracle as O
    c = cpu_bench.CONFIGS["deit_base"]
    for d in ("a", "b"):  # the same arguments twice: the same inputs, so the same files
        cpu_bench.main(["--gpus", "1", "--steps", "1", "--warmup", "0", "--dump-outputs", str(tmp_path / d)], run=_stub_run)
    got = {n: np.load(tmp_path / "a" / n) for n in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(got) == ["idx.npy", "images.npy", "out.npy"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert all(np.array_equal(a, np.load(tmp_path / "b" / n)) for n, a in got.items())
    assert got["images.npy"].tolist() == [0.0, 1.0, 2.0]  # the whole batch fits
    q, k, v, bias = cpu_bench.make_inputs(c, [0, 1, 2])
    r = O.attention(q, k, v, c["scale"], k_top=c["k"], pred_mode=c["mode"], bias=bias, flush=c["bias"])
    assert np.array_equal(got["out.npy"], r["out"]) and np.array_equal(got["idx.npy"], r["idx"])


def test_dump_outputs_samples_a_large_batch_within_its_byte_budget(cpu_bench, tmp_path, monkeypatch):
    """A batch above the budget: a seeded sample of its images, the same from run to run, every
    rank within its share."""
    out = torch.arange(7 * 2 * 5 * 4, dtype=torch.float32).reshape(7, 2, 5, 4)
    idx = torch.arange(7 * 2 * 5 * 3, dtype=torch.int64).reshape(7, 2, 5, 3)
    per_image = (2 * 5 * 4 + 2 * 5 * 3) * 4 + 8
    monkeypatch.setattr(cpu_bench, "DUMP_BYTES", 2 * 3 * per_image + 5)  # 3 images for each of 2 ranks
    images = list(range(10, 17))
    for d in ("a", "b"):
        cpu_bench.dump_outputs(str(tmp_path / d), out, idx, images, 1, 2)
    a = {n: np.load(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")}
    assert sorted(a) == ["idx_rank1.npy", "images_rank1.npy", "out_rank1.npy"]
    assert all(np.array_equal(v, np.load(tmp_path / "b" / n)) for n, v in a.items())
    sel = [images.index(int(i)) for i in a["images_rank1.npy"]]
    assert len(sel) == 3 and sel == sorted(set(sel))
    assert np.array_equal(a["out_rank1.npy"], out[sel].numpy()) and np.array_equal(a["idx_rank1.npy"], idx[sel].numpy())
    assert sum(v.nbytes for v in a.values()) <= cpu_bench.DUMP_BYTES // 2


@pytest.mark.gpu
def test_plain_run_on_the_gpu_times_the_steps_it_was_given_and_dumps_what_they_computed(tmp_path, monkeypatch, capsys):
    """The PixArt cross-attention config (3 images): --steps calls of the op inside the one
    timed region and no pass through the timed twin; the dumped idx equals the oracle's bit
    for bit and out is within the bench's parity tolerance."""
    import bench
    from mx_quantization_amd import _native as N
    from oracle import mx_oracle as O
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MXA_BENCH_BACKEND"):
        monkeypatch.delenv(var, raising=False)
    c = dict(bench.CONFIGS["pixart_cross"], B=3)
    monkeypatch.setitem(bench.CONFIGS, "pixart_cross", c)
    regions, real = [], bench.timed_region

    def no_twin(*a):
        raise AssertionError("a plain run went through mxa_attention_timed")
    monkeypatch.setattr(N.lib(), "mxa_attention_timed", no_twin)
    monkeypatch.setattr(bench, "timed_region",
                        lambda run, world, sync, device: real(lambda: regions.append(len(run())), world, sync, device))
    bench.main(["--config", "pixart_cross", "--gpus", "1", "--steps", "4", "--warmup", "1",
                "--dump-outputs", str(tmp_path)])
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert regions == [4] and line["steps"] == 4
    assert all(k in line for k in CONTRACT) and not any(k in line for k in FULL_ONLY)
    assert line["value"] == pytest.approx(3 * 256 * 4 / (line["ms_per_step"] * 4 / 1e3))
    out, idx, img = (np.load(tmp_path / f"{n}.npy") for n in ("out", "idx", "images"))
    assert out.dtype == np.float32 and idx.dtype == np.float32 and img.tolist() == [0.0, 1.0, 2.0]
    q, k, v, bias = bench.make_inputs(c, [0, 1, 2])
    r = O.attention(q, k, v, c["scale"], k_top=c["k"], pred_mode=c["mode"], bias=bias, flush=c["bias"])
    assert np.array_equal(idx, r["idx"])
    assert O.normwise_rel_err(out, r["out"]) <= 1e-3
