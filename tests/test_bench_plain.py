"""bench.py without a GPU: a plain run measures the headline and nothing else; --full adds the live traffic, the measured peak,
the secondary workloads, the restore / host-fed rates and the CPU baseline (Bench, CpuReference and live_traffic stood in for)."""
import json
import os

import pytest

import bench


def headline(cfg):
    return {"value": 1.0, "ms_per_step": 2.0, "ms_per_step_spread": {}, "workload": cfg["kind"], "min_avg_max": [1, 2, 3],
            "tree_bytes": 1, "files": 1, "jobs": 1, "bytes_this_rank": 1, "jobs_this_rank": 1, "roofline": None, "kernels": {},
            "phase_ms": {}, "result": dict.fromkeys(("chunks", "unique_chunks", "blocks", "raw_bytes_written", "gathered_blocks_rank0",
                                                    "gathered_bytes_rank0", "gather_GBps_rank0"), 0) | {"ratio": 1.0}}


@pytest.fixture
def calls(monkeypatch):
    calls = []

    class FakeBench:
        rank, world, comm_info, plain = 0, 1, None, False

        def __init__(self, args):
            pass

        def run(self, cfg, steps, warmup, dump_dir=None):
            calls.append(("run", cfg["tree"], cfg["kind"], cfg["codec"], steps, warmup, dump_dir))
            return headline(cfg)

        def measure_peak(self, gib):
            calls.append(("measure_peak",))

        def restore_rates(self):
            calls.append(("restore",))
            return {}

        def host_fed_rates(self):
            calls.append(("host_fed",))
            return {}

    class FakeCpuReference:
        ncpu, physical, quota, have_ref = 4, 2, None, False

        def __init__(self, b, args):
            calls.append(("cpu_reference",))

        def leg(self, cfg, gib, **kw):
            calls.append(("cpu_leg", cfg["kind"], cfg["codec"]))
            return {"value": 1.0}

        def close(self):
            pass

    monkeypatch.setattr(bench, "Bench", FakeBench)
    monkeypatch.setattr(bench, "CpuReference", FakeCpuReference)
    monkeypatch.setattr(bench, "live_traffic", lambda args: calls.append(("live_traffic",)))
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for k in [k for k in os.environ if k.startswith(("ROCP", "ROCPROF"))]:
        monkeypatch.delenv(k)
    return calls


def run_main(monkeypatch, capsys, *argv):
    monkeypatch.setattr("sys.argv", ["bench.py", *argv])
    bench.main()
    lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only(calls, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", "d")
    assert calls == [("run", "files", "random", "lz4", 7, 2, "d")]
    assert line["secondary"] is None and line["cpu_baseline"] is None
    assert (line["metric"], line["value"], line["unit"], line["higher_is_better"], line["dtype"], line["ms_per_step"]) == \
        ("ingest GB/s (chunk+hash+compress)", 1.0, "GB/s", True, "u8/u32", 2.0)


def test_full_run_adds_every_other_measurement(calls, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--gpus", "1", "--steps", "7", "--warmup", "2", "--full")
    names = [c[0] for c in calls]
    assert names[:3] == ["live_traffic", "measure_peak", "run"] and calls[2] == ("run", "files", "random", "lz4", 7, 2, None)
    assert {"cpu_reference", "cpu_leg", "restore", "host_fed"} <= set(names)
    assert names.count("run") == 7  # the headline and the six secondary workloads
    assert set(line["secondary"]) == {"compressible", "dedup", "north_star_tree", "north_star_tree_compressible", "zstd_compressible",
                                      "pak_zstd", "restore", "host_fed"}
    assert line["cpu_baseline"] == {"value": 1.0}
    assert line["value"] == 1.0 and line["ms_per_step"] == 2.0


def test_full_run_keeps_its_opt_outs(calls, monkeypatch, capsys):
    line = run_main(monkeypatch, capsys, "--full", "--no-secondary", "--no-cpu-baseline", "--no-live-traffic")
    assert [c[0] for c in calls] == ["measure_peak", "run"]
    assert line["secondary"] is None and line["cpu_baseline"] is None
