"""bench.py's roofline object and the issue model behind `valu.issue_model_frac`, checked on the CPU from the committed
profiles: the arithmetic the one-line JSON contract promises (achieved = algorithmic bytes / kernel time, frac = achieved /
peak, the VALU sub-object's fractions) and tools/cycle_probe.py's class-cost models of a ladder step."""
import importlib.util
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_issue_models_of_a_ladder_step():
    cp = load(os.path.join(ROOT, "tools", "cycle_probe.py"), "c25519_cycle_probe")
    mad, half, vop2 = cp.STEP_MAD, cp.STEP_HALF, cp.STEP_FULL
    assert (mad, half, vop2) == (739, 188, 319)                      # profiles/r04_isa_mix.txt, the ladder's loop
    n4 = mad + half
    assert cp.model_cycles("nominal") == 4 * n4 + 2 * vop2 == 4346
    assert abs(cp.model_cycles("measured_vop2_paired") - (4.26 * n4 + 2.13 * vop2)) < 1e-6
    # the floor: the VOP2 work first fills the 0.26-cycle bubble every 4-cycle-class instruction leaves at four waves
    floor = 4.26 * n4 + max(0.0, 2.13 * vop2 - 0.26 * n4)
    assert abs(cp.model_cycles("floor") - floor) < 1e-6 and 4380 < floor < 4395


def test_roofline_object_from_the_committed_measurements():
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench")
    n, ms = 1 << 20, 7.8
    probe = bench.issue_model(n, live=False)
    assert probe and "committed measurement" in probe["source"]
    r = bench.roofline_for("x25519", n, ms, probe)
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert r["algorithmic_bytes_per_launch"] == 96 * n                 # pk + sk in, shared key out
    assert abs(r["achieved"] - 96 * n / (ms * 1e-3) / 1e9) < 1e-2 and abs(r["frac"] - r["achieved"] / 8000.0) < 1e-6
    assert r["kernel"] == "k_x25519_ladder + k_batch_invert<FinishX25519>"
    v = r["valu"]
    assert abs(v["achieved"] * 1e12 - v["algorithmic_macs_per_op"] * n / (ms * 1e-3)) / (v["achieved"] * 1e12) < 1e-3
    assert abs(v["frac"] - v["achieved"] / v["peak"]) < 1e-3
    assert abs(v["frac_executed"] / v["frac"] - v["executed_macs_per_op"] / v["algorithmic_macs_per_op"]) < 1e-3
    assert 0.9 < v["issue_model_frac"] <= 1.02 and 4300 < v["simd_cycles_per_ladder_step"] < 5000
    assert v["ladder_step_instructions"] == {"v_mad_u64_u32": 739, "other_4_cycle_class": 188, "vop2": 319}
    # a batch the one-launch kernel runs names that kernel
    assert bench.roofline_for("x25519", 1 << 15, 0.7)["kernel"] == "k_x25519_fused"
    # traffic comes from the committed PMC passes of the same kernels, per pass
    with open(os.path.join(ROOT, "profiles", "r04_pmc.json")) as f:
        assert json.load(f)
    assert r["traffic"] is None or 2e8 < r["traffic"] < 4e8
    # the roof that binds is named at the top level, beside the contract's HBM fields
    assert r["binding"] == "valu" and r["binding_frac"] == v["frac"] and "two launches" in r["note"]
    assert r["traffic"] is None or abs(r["traffic_over_algorithmic"] - r["traffic"] / (96 * n)) < 0.01


def test_executed_macs_are_counted_from_the_device_source():
    """roofline.valu.executed_macs_per_op comes from profiles/rNN_executed_macs.json, which tools/executed_macs.py writes by
    running the device source on the C model of the gfx950 primitives and counting v_mad_u64_u32 / v_mad_i64_i32: a fresh count equals
    the committed file for all three passes, the ladder's count agrees with the ISA's 739 MADs per step
    (profiles/r04_isa_mix.txt, tools/cycle_probe.py), and bench.py uses the file."""
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_macs")
    em = load(os.path.join(ROOT, "tools", "executed_macs.py"), "c25519_executed_macs")
    cp = load(os.path.join(ROOT, "tools", "cycle_probe.py"), "c25519_cycle_probe_macs")
    fresh = em.count(sample=16)
    used, src = bench.executed_macs()
    assert src and src.endswith("_executed_macs.json")
    with open(os.path.join(ROOT, "profiles", src)) as f:
        committed = json.load(f)
    for k in ("x25519", "sign", "verify"):
        assert used[k] == committed["per_op"][k]
        assert abs(fresh["per_op"][k] - committed["per_op"][k]) <= 0.005 * committed["per_op"][k], (k, fresh["per_op"], committed["per_op"])
    d = fresh["detail"]
    assert (d["fe_mul"], d["fe_sq"]) == (101.0, 56.0)                 # 100 / 55 in the asm chains + the x19 fold
    assert abs(d["x25519_ladder"] / cp.STEPS - cp.STEP_MAD) < 0.005 * cp.STEP_MAD
    # executed <= the reference's algorithmic count for the re-designed passes, a few per cent above it for the ladder
    assert 1.0 < used["x25519"] / bench.MACS_PER_OP["x25519"] < 1.05
    assert used["sign"] < 0.5 * bench.MACS_PER_OP["sign"] and used["verify"] < 0.8 * bench.MACS_PER_OP["verify"]


def test_valu_issue_figures_are_the_counter_files_arithmetic():
    """roofline.*.valu.issue (north_star: "VALU-busy against chip peak"): per kernel of a pass, from the committed
    rocprofv3 counter passes and the committed instruction classes of the kernels' hot loops (tools/valu_issue.py) -- recomputed
    here by hand from the same two files, for the ladder, the verification walk and points kernels and the signing walk."""
    import glob
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_issue")
    vi = load(os.path.join(ROOT, "tools", "valu_issue.py"), "c25519_valu_issue")
    pmc_path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_pmc.json")))[-1]
    cls_path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_isa_classes.json")))[-1]
    with open(pmc_path) as f:
        pmc = json.load(f)
    with open(cls_path) as f:
        cls = json.load(f)
    seen = 0
    for wl in ("x25519", "verify", "sign"):
        got = bench.valu_issue(bench.PASS_KERNELS[wl])
        assert got and os.path.basename(pmc_path) in got["source"] and os.path.basename(cls_path) in got["source"]
        cyc = busy = 0.0
        for k, r in got["per_kernel"].items():
            rec = vi.find(pmc, k)
            simd_cycles = rec["GRBM_GUI_ACTIVE"] / 8                       # shader cycles the dispatch was resident, per XCD
            per_simd = rec["SQ_INSTS_VALU"] / 1024
            assert abs(r["simd_cycles"] - simd_cycles) <= 1 and abs(r["valu_insts_per_simd"] - per_simd) <= 1
            assert abs(r["valu_busy"] - rec["SQ_ACTIVE_INST_VALU"] * 4 / (1024 * simd_cycles)) < 1e-3
            c = vi.find(cls, k)
            if c:
                m = c.get("hot_loop") or c["whole_kernel"]
                assert m["mad64"] + m["other_four_cycle"] + m["vop2"] == m["valu"]
                n2 = per_simd * m["vop2"] / m["valu"]
                assert abs(r["valu_issue_util"] - ((per_simd - n2) * 4 + n2 * 2) / simd_cycles) < 1e-3
                assert 0.3 < r["valu_issue_util"] < 1.05
                seen += 1
            cyc += simd_cycles
            busy += r["valu_busy"] * simd_cycles
        assert abs(got["valu_busy"] - busy / cyc) < 1e-3
    assert seen >= 5                                                       # ladder, walk, points, scalars, sign_mult, ...
    # the ladder's loop in the committed classes is the loop the issue model prices (739 MADs per step)
    assert vi.find(cls, "k_x25519_ladder")["hot_loop"]["mad64"] == 739


def test_live_peak_replaces_the_committed_one_and_keeps_it_beside():
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_live")
    r = bench.roofline_for("sign", 1 << 20, 1.25)
    v = dict(r["valu"])
    committed, frac0 = v["peak"], v["frac"]
    bench.apply_live_peak(v, {"v_mad_u64_u32": 36.0e12})
    assert v["peak"] == v["peak_live"] == 36.0 and v["peak_committed"] == committed and v["frac_vs_committed_peak"] == frac0
    assert abs(v["frac"] - v["achieved"] / 36.0) < 1e-3 and v["peak_policy"].startswith("live")
    assert abs(v["frac_executed"] / v["frac"] - v["executed_macs_per_op"] / v["algorithmic_macs_per_op"]) < 1e-3
    w = dict(r["valu"])
    bench.apply_live_peak(w, None)                                         # no live measurement: the committed peak, said so
    assert w["peak"] == committed and w["peak_live"] is None and w["frac"] == frac0 and w["peak_policy"].startswith("committed")


def test_expected_digests_cover_every_rank_of_the_scaling_run():
    """bench.py attests bit-exactness per rank from tests/golden/digests.json["ranks"] (the reference's outputs for each
    rank's seeded inputs): ranks 0..7 at 2^20 and the power-of-two prefixes its tests run at; rank 0 of any world and the
    lone rank of a world of one share the unshifted seed, i.e. the digests the parity tests already pin."""
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_digests")
    with open(os.path.join(ROOT, "tests", "golden", "digests.json")) as f:
        dig = json.load(f)
    n = 1 << 20
    seen = set()
    for r in range(8):
        e = bench.expected_digests(r, 8, n)
        assert e and len(e["x25519_shared"]) == 64 and set(e["mixed_thirds"]) >= {"x25519_shared", "ed25519_sig", "ed25519_verdicts"}
        seen.add(e["x25519_shared"])
        for m in (1 << 14, 1 << 16):
            assert bench.expected_digests(r, 8, m)
    assert len(seen) == 8                                              # every rank has inputs of its own
    assert bench.expected_digests(0, 1, n) == bench.expected_digests(0, 8, n)
    for k, v in dig[str(n)].items():
        assert k == "n" or bench.expected_digests(0, 1, n)[k] == v
    assert bench.expected_digests(0, 1, 12345) is None and bench.expected_digests(9, 16, n) is None


def test_rank_attestation_says_what_rccl_saw():
    """The line's `ranks` / `rccl` objects (rccl.h:745): N ranks on N distinct devices over the "nccl" backend is
    the only thing that counts as a multi-GPU measurement; a shared device, a gloo group or the logical devices of one
    partitioned MI355X say so."""
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_attest")
    def ident(r, uuid, pci, idx, part=None):
        return {"rank": r, "uuid": uuid, "pci_bus_id": pci, "device_index": idx, "compute_partition": part}
    eight = [ident(r, f"GPU-{r:02x}", f"0000:{0x10 + r:02x}:00", r) for r in range(8)]
    a = bench.attest_ranks(eight, 8, "nccl", False)
    assert a["devices_distinct"] and a["devices_distinct_by_uuid_or_pci"] and a["is_multi_gpu_measurement"]
    assert a["world"] == 8 and a["ranks_seen"] == 8 and not a["compute_partitions_of_one_device"]
    same = [ident(r, "GPU-00", "0000:10:00", 0) for r in range(2)]
    a = bench.attest_ranks(same, 2, "gloo", True)
    assert not a["devices_distinct"] and not a["is_multi_gpu_measurement"] and a["shared_gpu_selftest"]
    assert not bench.attest_ranks(same, 2, "nccl", False)["devices_distinct"]          # main() refuses to run this
    cpx = [ident(r, f"GPU-{r:02x}", "0000:10:00", r) for r in range(8)]              # eight logical devices of ONE package
    a = bench.attest_ranks(cpx, 8, "nccl", False)
    assert a["devices_distinct"] and a["compute_partitions_of_one_device"] and not a["is_multi_gpu_measurement"]
    one = bench.attest_ranks([ident(0, "GPU-00", "0000:10:00", 0)], 1, None, False)
    assert one["devices_distinct"] and not one["is_multi_gpu_measurement"] and one["backend"] is None


def test_the_committed_line_carries_the_mid_size_and_single_call_figures():
    """The round's work where the driver records it (VERDICT r05 missing #2 / #3): calls of 2^12 / 2^14 elements and ONE call through
    the reference's prototypes are measured by bench.py itself (`extra.mid_size_calls`, `extra.single_call_us`), checked for
    correctness in the same run, and the committed line of the round has them."""
    import glob
    path = sorted(glob.glob(os.path.join(ROOT, "profiles", "r[0-9][0-9]_bench.json")))[-1]
    line = json.loads([l for l in open(path) if l.startswith("{")][-1])
    mid, one = line["extra"]["mid_size_calls"], line["extra"]["single_call_us"]
    for op in ("x25519", "sign", "verify"):
        for size in ("2^12", "2^14"):
            rec = mid[op][size]
            assert rec["ms_per_call"] > 0 and abs(rec["per_s"] * rec["ms_per_call"] * 1e-3 / (1 << int(size[2:])) - 1) < 1e-3
    assert mid["verify"]["2^12"]["all_valid"] and mid["verify"]["2^14"]["all_valid"]
    assert mid["x25519"]["2^14"]["per_s"] > 4 * 9.6e6 and mid["sign"]["2^12"]["per_s"] > 2 * 22.8e6       # round 5: 2^12 X25519 9.6 M/s, 2^12 signatures 22.8 M/s
    assert one["bytes_equal_the_batch"] is True
    assert one["curve25519_dh_CreateSharedKey"] < 168 and one["ed25519_SignMessage"] < 105 and one["ed25519_VerifySignature"] < 135   # round 5's


def test_dump_outputs_writes_exact_seeded_samples(tmp_path):
    """--dump-outputs: one .npy per output, float32 for bytes and float64 for 32-bit words (exact), all rows of a small
    output, a seeded sample of 2^16 rows (and their indices) of a large one -- the same rows in every run -- and 64 MB at most."""
    import numpy as np
    bench = load(os.path.join(ROOT, "bench.py"), "c25519_bench_dump")
    rng = np.random.default_rng(7)
    big = rng.integers(0, 256, (1 << 20, 64), dtype=np.uint8)
    words = rng.integers(0, 2, (1 << 20, 1), dtype=np.int32)
    small = rng.integers(0, 256, (1000, 32), dtype=np.uint8)
    arrays = [("sign_signatures", big), ("verify_verdicts", words), ("x25519_shared", small)]
    files = bench.dump_outputs(str(tmp_path / "a"), arrays)
    assert sorted(files) == sorted(["sign_signatures.npy", "sign_signatures_rows.npy", "verify_verdicts.npy",
                                    "verify_verdicts_rows.npy", "x25519_shared.npy"])
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in files)
    assert total <= 64 << 20
    sig, rows = np.load(tmp_path / "a" / "sign_signatures.npy"), np.load(tmp_path / "a" / "sign_signatures_rows.npy")
    assert sig.dtype == np.float32 and sig.shape == (1 << 16, 64) and rows.dtype == np.float64
    assert np.all(np.diff(rows) > 0) and np.array_equal(sig, big[rows.astype(np.int64)].astype(np.float32))
    ok = np.load(tmp_path / "a" / "verify_verdicts.npy")
    assert ok.dtype == np.float64 and np.array_equal(ok, words[np.load(tmp_path / "a" / "verify_verdicts_rows.npy").astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "a" / "x25519_shared.npy"), small.astype(np.float32))
    bench.dump_outputs(str(tmp_path / "b"), arrays)                   # another run, the same inputs: the same files
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f


def test_bench_steps_must_be_positive():
    import subprocess
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + bad, capture_output=True, text=True, timeout=120)
        assert p.returncode == 2 and "--steps must be at least 1" in p.stderr, (bad, p.stderr[-1000:])
