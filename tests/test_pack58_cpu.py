"""The 58-bit row format (csrc/kernels/pack58.h) against a NumPy model written from its description.

The model packs a row through Python integers (one 416-bit number per lane for the high plane), so it shares
no code and no bit tricks with the header.  The header's host functions (pack_row / unpack_row, the same
encode / decode / field_of the packer and the gradient kernel call) are built into a stand-alone program with
-fsanitize=address,undefined and compared with the model byte for byte.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROW_BYTES, WINDOW = 7424, 31
E0 = 1023 - 24  # the window [2^-24, 2^7): what N(0, 1) data picks, more or less


def model_pack(x: np.ndarray, e0: int):
    """(7424 bytes, exact) of one row of at most 1024 doubles."""
    u = np.zeros(1024, dtype=np.uint64)
    u[: x.size] = x.view(np.uint64)
    blob = np.zeros(ROW_BYTES // 4, dtype=np.uint32)
    exact = True
    for lane in range(64):
        big = 0
        for k in range(16):
            c = ((k // 2) * 64 + lane) * 2 + k % 2
            v = int(u[c])
            sign, e, mant = v >> 63, (v >> 52) & 0x7FF, v & ((1 << 52) - 1)
            if e0 <= e <= e0 + WINDOW - 1:
                field, low = (sign << 25) | ((e - e0 + 1) << 20) | (mant >> 32), mant & 0xFFFFFFFF
            else:
                field, low = sign << 25, 0  # code 0 is +-0
                exact = exact and e == 0 and mant == 0
            big |= field << (26 * k)
            blob[(k // 4) * 256 + lane * 4 + k % 4] = low
        for w in range(12):
            blob[1024 + (w // 4) * 256 + lane * 4 + w % 4] = (big >> (32 * w)) & 0xFFFFFFFF
        blob[1024 + 768 + lane] = (big >> (32 * 12)) & 0xFFFFFFFF
    return blob.view(np.uint8), exact


def model_unpack(blob: np.ndarray, ld: int, e0: int) -> np.ndarray:
    w32 = blob.view(np.uint32)
    out = np.zeros(1024, dtype=np.uint64)
    for lane in range(64):
        big = sum(int(w32[1024 + (w // 4) * 256 + lane * 4 + w % 4]) << (32 * w) for w in range(12))
        big |= int(w32[1024 + 768 + lane]) << (32 * 12)
        for k in range(16):
            f = (big >> (26 * k)) & 0x3FFFFFF
            sign, code, mh = f >> 25, (f >> 20) & 31, f & 0xFFFFF
            low = int(w32[(k // 4) * 256 + lane * 4 + k % 4])
            v = (sign << 63) | ((((code + e0 - 1) << 52) | (mh << 32) | low) if code else 0)
            out[((k // 2) * 64 + lane) * 2 + k % 2] = v
    return out[:ld].view(np.float64)


def bits(sign: int, e: int, mant: int) -> float:
    return np.array([(sign << 63) | (e << 52) | mant], dtype=np.uint64).view(np.float64)[0]


FULL = (1 << 52) - 1


def rows(ld: int):
    """[(name, row, exact)]: every row N(0, 1) noise inside the window plus the planted values."""
    rng = np.random.default_rng(ld)
    base = np.clip(np.abs(rng.standard_normal(ld)), 2.0 ** -20, 60.0) * rng.choice([-1.0, 1.0], ld)
    cases = {
        "noise": ([], True),
        "zeros": ([0.0, -0.0], True),
        "low edge": ([bits(0, E0, 0), bits(1, E0, FULL), bits(0, E0, 1)], True),
        "high edge": ([bits(0, E0 + 30, FULL), bits(1, E0 + 30, 0), bits(1, E0 + 30, 1 << 32)], True),
        "mantissas": ([bits(0, 1023, FULL), bits(1, 1023, 0), bits(0, 1020, 0xFFFFFFFF), bits(0, 1020, 1 << 51)], True),
        "below": ([bits(0, E0 - 1, FULL)], False),
        "above": ([bits(1, E0 + 31, 0)], False),
        "denormal": ([bits(0, 0, 1)], False),
        "largest denormal": ([bits(1, 0, FULL)], False),
        "inf": ([np.inf], False),
        "-inf": ([-np.inf], False),
        "nan": ([np.nan], False),
    }
    out = []
    for name, (vals, exact) in cases.items():
        for where in ("front", "back"):
            r = base.copy()
            if vals:
                at = np.arange(len(vals)) if where == "front" else ld - 1 - np.arange(len(vals))
                r[at] = vals
            out.append((f"{name} {where}", r, exact))
    return out


@pytest.mark.parametrize("ld", [1000, 520])
def test_model_round_trip_and_flags(ld):
    for name, r, exact in rows(ld):
        blob, ok = model_pack(r, E0)
        assert ok == exact, name
        back = model_unpack(blob, ld, E0)
        if exact:
            assert np.array_equal(back.view(np.int64), r.view(np.int64)), name
        else:
            assert not np.array_equal(back.view(np.int64), r.view(np.int64)), name
        # pad columns (and pad lanes at d = 520) are code 0 with a zero low word
        full = model_unpack(blob, 1024, E0)
        assert not full[ld:].view(np.int64).any(), name


@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("pack58") / "pack58_host")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "csrc"),
           os.path.join(ROOT, "tests", "pack58_host.cpp"), "-o", exe]
    san = subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if san.returncode != 0:  # a toolchain without the sanitizer runtimes still checks the header against the model
        subprocess.run(cmd, check=True)
    return exe


@pytest.mark.parametrize("ld", [1000, 520])
def test_header_matches_the_model(host_program, tmp_path, ld):
    cases = rows(ld)
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(src, "wb") as f:
        f.write(struct.pack("<iii", ld, E0, len(cases)))
        for _, r, _ in cases:
            f.write(r.tobytes())
    done = subprocess.run([host_program, str(src), str(dst)], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    raw = np.fromfile(dst, dtype=np.uint8)
    rec = ROW_BYTES + 1 + 8 * ld
    assert raw.size == rec * len(cases)
    for i, (name, r, exact) in enumerate(cases):
        blob, flag, back = np.split(raw[i * rec: (i + 1) * rec], [ROW_BYTES, ROW_BYTES + 1])
        want, ok = model_pack(r, E0)
        assert ok == exact and bool(flag[0]) == exact, name
        assert np.array_equal(blob, want), name
        assert np.array_equal(back.view(np.int64), model_unpack(want, ld, E0).view(np.int64)), name
        assert np.array_equal(back.view(np.int64), r.view(np.int64)) == exact, name


def test_packed_kernels_of_the_default_picks_do_not_spill(tmp_path):
    """Every (loss, replicas) the long-stream rule can pack: its grad_dense_p58 instance exists, keeps no
    register in scratch memory and fits one workgroup per CU (512 registers per lane at one wave per SIMD)."""
    from test_isa_checks import READELF, _code_objects, _kernel_regs

    from erasurehead_amd.ops.grad import choose_kernel

    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    regs = {}
    for co in _code_objects(tmp_path):
        regs.update(_kernel_regs(co))
    assert any("pack58_bundles" in n for n in regs)
    for rep in (1, 2, 3):
        c = choose_kernel(0, 1000, 16, rep, 10 ** 6)
        assert c.kind == "multi" and c.fold and not c.pair, c
        for loss in (0, 1, 2):
            key = f"grad_dense_p58ILi{loss}ELi{rep}ELi{int(c.lane_epi)}E"
            hit = [r for n, r in regs.items() if key in n]
            assert len(hit) == 1, key
            assert hit[0][1] == 0 and hit[0][0] <= 512, (key, hit[0])


def test_window_choice_and_plan_rule():
    import torch

    from erasurehead_amd.ops.grad import (LONG_STREAM_ROWS_PER_CU, N_CUS, KernelChoice, choose_kernel, pack58_window,
                                          pack_auto, pack_eligible)

    X = torch.from_numpy(np.random.default_rng(0).standard_normal((64, 1000)))
    e0 = pack58_window(X)
    e = (X.numpy().view(np.int64) >> 52) & 0x7FF
    held = lambda a: int(((e >= a) & (e <= a + 30)).sum())
    assert held(e0) == max(held(a) for a in range(e0 - 40, e0 + 40)) and held(e0) > 0.999 * e.size
    assert pack58_window(X * 2.0 ** 200) == e0 + 200
    assert pack58_window(torch.zeros(4, 1000, dtype=torch.float64)) == 1
    c = choose_kernel(0, 1000, 16, 3, 10 ** 6)
    assert pack_eligible(c, 0, 1000, 16) and pack_eligible(c, 0, 520, 16)
    for code in (1, 2, 3):  # fp32, bf16, fp32x64 rows stay plain
        assert not pack_eligible(c, code, 1000, 16)
    assert not pack_eligible(c, 0, 512, 8) and not pack_eligible(c, 0, 1026, 32)
    assert not pack_eligible(KernelChoice("multi", replicas=3, bundle_rows=32), 0, 1000, 16)  # not folded
    assert not pack_eligible(KernelChoice("staged", replicas=3, bundle_rows=32), 0, 1000, 16)
    assert pack_auto(10 ** 6) and pack_auto(LONG_STREAM_ROWS_PER_CU * N_CUS)
    assert not pack_auto(500_000)  # the N = 2 rank shape and everything smaller stays plain
    assert pack_auto(500_000, n_cus=128)  # a rows-per-CU rule
