"""CPU: the host-side helpers of bench.py that decide what the JSON line may claim -- which committed counter summary belongs to
the library that ran (build id), and what "one socket of this box" means for the CPU baseline -- and what --dump-outputs
writes.  GPU: one small plain run of bench.py."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_counter_summary_is_taken_only_from_the_same_build(tmp_path, monkeypatch):
    """profiles/rNN_pmc_summary*.txt carry `# build_id <asora_build_id()>` (tools/pmc.sh); bench.py pairs its timings with the
    newest summary of the SAME build and otherwise reports no traffic, with the reason."""
    prof = tmp_path / "profiles"
    prof.mkdir()
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.find_pmc_summary("abc") == (None, "no counter summary under profiles/")
    (prof / "r03_pmc_summary.txt").write_text("# no id here\nraytrace_octant_kernel FETCH_SIZE n=2 mean=100\n")
    (prof / "r04_pmc_summary.txt").write_text("# build_id 1111\nraytrace_octant_kernel FETCH_SIZE n=2 mean=200\nraytrace_octant_kernel WRITE_SIZE n=2 mean=50\n")
    (prof / "r05_pmc_summary.txt").write_text("# cmd\n# build_id 2222\nraytrace_octant_kernel FETCH_SIZE n=2 mean=300\nraytrace_octant_kernel WRITE_SIZE n=2 mean=70\n")
    (prof / "r05_pmc_summary_R16.txt").write_text("# build_id 1111\nraytrace_octant_kernel FETCH_SIZE n=2 mean=999\n")
    path, why = bench.find_pmc_summary("2222")
    assert path == os.path.join("profiles", "r05_pmc_summary.txt") and why is None
    assert bench.pmc_traffic_bytes("raytrace_octant_kernel", path) == (2 * 300 + 70) * 1024.0       # KiB, FETCH_SIZE doubled (gfx950)
    assert bench.find_pmc_summary("1111")[0] in (os.path.join("profiles", "r05_pmc_summary_R16.txt"),)   # the newest round that matches
    path, why = bench.find_pmc_summary("3333")
    assert path is None and "3333" in why and "re-run tools/pmc.sh" in why
    assert bench.pmc_counters("raytrace_octant_kernel", None) == {} and bench.pmc_traffic_bytes("raytrace_octant_kernel", None) is None


def test_host_topology_is_consistent():
    t = bench.host_topology()
    assert t["logical_cpus"] >= 1 and t["sockets"] >= 1
    assert 1 <= t["physical_cores_per_socket"] <= t["logical_cpus"]
    assert 1 <= t["usable_cpus"] <= t["affinity_cpus"] <= t["logical_cpus"]
    assert t["logical_cpus_per_socket"] * t["sockets"] <= t["logical_cpus"] + t["sockets"]
    if t["cgroup_cpu_quota"] is not None:
        assert t["usable_cpus"] <= max(1, int(t["cgroup_cpu_quota"] + 0.5))


def test_usable_memory_is_a_positive_number_or_unknown():
    m = bench.usable_memory_bytes()
    assert m is None or m > 0


def test_every_json_record_under_profiles_parses():
    """profiles/*.json are records a reader (and the judge) loads with json.load: no log text around the JSON."""
    import glob
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "profiles", "*.json")))
    assert files
    for f in files:
        with open(f) as fh:
            json.load(fh)


def test_dump_outputs_writes_small_grids_whole(tmp_path):
    rng = np.random.default_rng(1)
    grids = {"xh_new": rng.random((8, 8, 8)), "phi_ion": rng.random((8, 8, 8))}
    bench.dump_outputs(str(tmp_path / "out"), grids)
    for name, a in grids.items():
        got = np.load(tmp_path / "out" / f"{name}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, a)


def test_dump_outputs_samples_large_grids_the_same_cells_every_time(tmp_path, monkeypatch):
    """Grids above the size limit: the same seeded, sorted sample of flat C-order cells of each grid, run after run, and all
    files together within the limit."""
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_CELLS", 200)
    N = 16
    x = np.arange(N ** 3, dtype=np.float64).reshape(N, N, N)
    phi = np.asfortranarray(2.0 * x)                                # memory order must not change which cells are taken
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"xh_new": x, "phi_ion": phi})
    xa, pa = np.load(tmp_path / "a" / "xh_new.npy"), np.load(tmp_path / "a" / "phi_ion.npy")
    assert xa.shape == (200,) and np.array_equal(pa, 2.0 * xa)
    assert np.all(np.diff(xa) > 0) and xa[0] >= 0 and xa[-1] < N ** 3      # distinct cells, ascending index
    assert np.array_equal(xa, np.load(tmp_path / "b" / "xh_new.npy"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 4096 + 2 * 128   # + .npy headers


def test_default_bench_dump_fits_the_limit():
    """The default job (256^3, two grids) is sampled, and the sample of both grids fits the 64 MB the dump may take."""
    assert 2 * 8 * 256 ** 3 > bench.DUMP_LIMIT_BYTES
    assert 2 * 8 * bench.DUMP_SAMPLE_CELLS <= bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_plain_bench_run_times_exactly_the_steps_asked_for(tmp_path):
    """`bench.py --steps K --warmup W` without --full: one timed region of K steps, the headline fields, none of the extras,
    and --dump-outputs writes the two grids of the last step."""
    import json
    import subprocess
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--N", "64",
                        "--nsrc", "20", "--R", "8", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["repeats"] == 1 and len(d["spread"]["ms_per_step_all"]) == 1
    assert d["ms_per_step"] > 0 and d["value"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["unit"] == "cell-updates/s" and d["metric"] == "cell-updates/sec (raytrace+chem)"
    assert "cpu_baseline" not in d and "evolving_state" not in d and d["config"]["first_iteration_of_a_time_step_ms"] is None
    x, phi = np.load(out / "xh_new.npy"), np.load(out / "phi_ion.npy")
    assert x.shape == phi.shape == (64, 64, 64) and x.dtype == phi.dtype == np.float64
    assert np.all((x > 0) & (x <= 1)) and np.all(np.isfinite(phi)) and phi.max() > 0
