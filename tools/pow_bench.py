#!/usr/bin/env python3
"""Measurement of the proof-of-work search (cs/implementations/pow.rs) for both runners, Blake2s256
and Keccak256, on the prover's seed shape (40 bytes: 5 field elements, prover.rs:2115-2118).

* "run_ms": the wall time of bj_pow_run_h (PoWRunner::run_from_bytes: midstate, launches, one
  8-byte copy and one synchronise per window) at `pow_bits` over `n_seeds` fixed seeds, after one
  untimed call: mean, standard deviation, least and most, and the mean of the nonces found.
* "rate_ghs": the raw hash rate, from bj_pow_search_d over consecutive windows of 2^28 nonces at
  pow_bits = 32, each launch between two device events on a result word of its own, as many
  launches as fill about 0.4 s.  A launch in whose window a nonce passed 32 bits stops early; it
  is counted in "launches_cut_short" and left out of the rate.
* "fraction_of_slot_floor": that rate over the VALU issue-slot floor of DESIGN.md section 4.1,
  78.6 T lane-slots/s over the slots of one hash.  The slots are counted in the compiler's assembly of the
  40-byte kernels the way tools/valu_census.py counts (full-rate instructions 1, the others 2):
  the search loop's body once, the Keccak rounds loop in it 22 times.

Every nonce reported is checked here with hashlib.blake2s or a pure-Python Keccak-f; the tool exits
non-zero on a mismatch.  `python tools/pow_bench.py 32 1` is the run that exercises a passing
nonce at 32 bits.

usage: python tools/pow_bench.py [pow_bits=20] [n_seeds=32] [--census FILE]   (prints one JSON line)
  --census FILE: read the slot counts from FILE if it exists, else count them and write FILE
  --census-only: count, print (and write) the slot counts and stop; needs no GPU
"""
import argparse
import ctypes
import hashlib
import json
import os
import re
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "era-boojum_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK_LANE_SLOTS = 256 * 4 * 32 * 2.4e9
RATE_WINDOW = 1 << 28
RATE_SECONDS = 0.4
HASHERS = {"blake2s": 1, "keccak256": 2}  # BJ_HASHER_*
KERNELS = {"blake2s": ("B2sPowELi1ELb1E", ()), "keccak256": ("KcPowELi1ELb1E", (22,))}
NO_RESULT = (1 << 64) - 1


# ------------------------------------------------------------------ the check

_RC = []
_r = 1
for _ in range(24):
    _c = 0
    for _j in range(7):
        if _r & 1:
            _c |= 1 << ((1 << _j) - 1)
        _r = ((_r << 1) ^ (0x71 if _r & 0x80 else 0)) & 0xFF
    _RC.append(_c)
_ROT = [[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]]
_M64 = (1 << 64) - 1


def _rol(v, n):
    return ((v << n) | (v >> (64 - n))) & _M64 if n else v


def keccak_f(a):
    """Keccak-f[1600] (FIPS 202 section 3.2) on a[x][y]."""
    for rc in _RC:
        c = [a[x][0] ^ a[x][1] ^ a[x][2] ^ a[x][3] ^ a[x][4] for x in range(5)]
        d = [c[(x + 4) % 5] ^ _rol(c[(x + 1) % 5], 1) for x in range(5)]
        a = [[a[x][y] ^ d[x] for y in range(5)] for x in range(5)]
        b = [[0] * 5 for _ in range(5)]
        for x in range(5):
            for y in range(5):
                b[y][(2 * x + 3 * y) % 5] = _rol(a[x][y], _ROT[x][y])
        a = [[b[x][y] ^ (~b[(x + 1) % 5][y] & b[(x + 2) % 5][y]) for y in range(5)] for x in range(5)]
        a[0][0] ^= rc
    return a


def keccak256(data):
    """Keccak256: rate 136, pad10*1 with domain byte 0x01 (not SHA3's 0x06)."""
    data = bytearray(data) + b"\x01"
    data += b"\x00" * (-len(data) % 136)
    data[-1] |= 0x80
    a = [[0] * 5 for _ in range(5)]
    for at in range(0, len(data), 136):
        for i in range(17):
            a[i % 5][i // 5] ^= int.from_bytes(data[at + 8 * i: at + 8 * i + 8], "little")
        a = keccak_f(a)
    return b"".join(a[i % 5][i // 5].to_bytes(8, "little") for i in range(4))


def passes(name, seed, pow_bits, nonce):
    """pow.rs:126-134: u64::from_le_bytes(digest[..8]).trailing_zeros() >= pow_bits."""
    data = seed + nonce.to_bytes(8, "little")
    digest = hashlib.blake2s(data, digest_size=32).digest() if name == "blake2s" else keccak256(data)
    return int.from_bytes(digest[:8], "little") & ((1 << pow_bits) - 1) == 0


def fixed_seed(i):
    return hashlib.shake_128(b"pow_bench seed %d" % i).digest(40)


# ------------------------------------------------------------------ the slot census

HIPCC = "/opt/rocm/bin/hipcc"
HIPFLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-munsafe-fp-atomics"]  # era-boojum_amd/Makefile


def census():
    """{"blake2s" | "keccak256": {"valu_per_hash", "slots_per_hash"}} of the 40-byte kernels, from
    the compiler's assembly of csrc/pow.hip.  Every basic block there carries its loop depth: 1
    the tile loop, 2 the search loop (one hash per trip), 3 a rounds loop inside the hash."""
    from valu_census import FULL_RATE
    asm = "/tmp/_pow_census.s"
    subprocess.run([HIPCC] + HIPFLAGS + ["--cuda-device-only", "-S", "-o", asm,
                                         os.path.join(ROOT, "era-boojum_amd", "csrc", "pow.hip")], check=True)
    out = {}
    for name, (tmpl, trips) in KERNELS.items():
        valu = slots = 0
        on, depth, fresh, rounds_loops = False, 0, False, []
        for line in open(asm):
            if re.match(r"^_Z\S*pow_search_kernel\S*:", line):
                on = tmpl in line
                depth = 0
                continue
            if not on:
                continue
            if line.startswith(".Lfunc_end"):
                break
            label = re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", line)
            if label:
                depth, fresh = 0, True
            text = line.strip()
            if label or (fresh and text.startswith(";")):
                m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)|in Loop: Header=\S+ Depth=(\d+)", line)
                if m:
                    depth = int(m.group(1) or m.group(2))
                    if m.group(1) and depth == 3:
                        rounds_loops.append(label.group(1) if label else "?")
                continue
            fresh = False
            mn = text.split()[0] if text else ""
            if depth < 2 or not mn.startswith("v_"):
                continue
            if depth > 3 or (depth == 3 and not trips):
                raise SystemExit("%s: a loop the census does not know, depth %d" % (name, depth))
            w = trips[len(rounds_loops) - 1] if depth == 3 else 1
            valu += w
            slots += w * (1 if FULL_RATE.match(mn) else 2)
        if not valu or len(rounds_loops) != len(trips):
            raise SystemExit("%s: kernel %s not found, or %d rounds loops where %d were expected"
                             % (name, tmpl, len(rounds_loops), len(trips)))
        out[name] = {"valu_per_hash": valu, "slots_per_hash": slots}
    return out


# ------------------------------------------------------------------ the measurements

def run_times(lib, torch, name, pow_bits, n_seeds):
    hasher = HASHERS[name]
    out = ctypes.c_uint64(0)

    def run(seed):
        t0 = time.perf_counter()
        rc = lib.bj_pow_run_h(hasher, seed, len(seed), pow_bits, ctypes.byref(out))
        t1 = time.perf_counter()
        if rc:
            raise SystemExit("bj_pow_run_h failed (%d): %s" % (rc, lib.bj_last_error().decode()))
        if out.value == NO_RESULT or not passes(name, seed, pow_bits, out.value):
            raise SystemExit("%s: nonce %d of seed %s does not pass %d bits" % (name, out.value, seed.hex(), pow_bits))
        return t1 - t0, out.value

    run(fixed_seed(10 ** 6))  # untimed: the thread's stream, the pool, the code object
    ms, nonces = [], []
    for i in range(n_seeds):
        t, nonce = run(fixed_seed(i))
        ms.append(t * 1e3)
        nonces.append(nonce)
    return {"run_ms_mean": statistics.mean(ms), "run_ms_stdev": statistics.pstdev(ms), "run_ms_min": min(ms),
            "run_ms_max": max(ms), "run_ms_median": statistics.median(ms), "nonce_mean": statistics.mean(nonces),
            "nonce_max": max(nonces), "nonces_checked": len(nonces)}


def hash_rate(torch, W, name):
    hasher, seed = HASHERS[name], fixed_seed(0)
    st = torch.cuda.current_stream()

    def launches(first, count):
        res = torch.full((count,), -1, dtype=torch.int64, device="cuda")   # BJ_POW_NO_RESULT each
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(count + 1)]
        torch.cuda.synchronize()
        ev[0].record(st)
        for i in range(count):
            W.search(hasher, seed, 32, first + i * RATE_WINDOW, RATE_WINDOW, res[i: i + 1])
            ev[i + 1].record(st)
        torch.cuda.synchronize()
        found = [int(v) & NO_RESULT for v in res.cpu()]
        return [ev[i].elapsed_time(ev[i + 1]) for i in range(count)], found

    warm, _ = launches(0, 2)
    count = max(4, min(256, int(RATE_SECONDS * 1e3 / warm[1]) + 1))
    ms, found = launches(2 * RATE_WINDOW, count)
    for i, nonce in enumerate(found):
        if nonce != NO_RESULT and not passes(name, seed, 32, nonce):
            raise SystemExit("%s: nonce %d of the rate run does not pass 32 bits" % (name, nonce))
    whole = [t for t, nonce in zip(ms, found) if nonce == NO_RESULT]
    if not whole:
        raise SystemExit("%s: every rate launch was cut short" % name)
    return {"rate_ghs": len(whole) * RATE_WINDOW / (sum(whole) * 1e-3) / 1e9, "rate_window": RATE_WINDOW,
            "launches": count, "launches_cut_short": count - len(whole), "timed_ms": sum(whole),
            "launch_ms_min": min(whole), "launch_ms_max": max(whole)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("pow_bits", nargs="?", type=int, default=20)
    ap.add_argument("n_seeds", nargs="?", type=int, default=32)
    ap.add_argument("--census")
    ap.add_argument("--census-only", action="store_true")
    args = ap.parse_args()
    if not 1 <= args.pow_bits <= 32 or args.n_seeds < 1:
        raise SystemExit("pow_bits 1..32, n_seeds >= 1")
    if args.census and os.path.exists(args.census):
        slots = json.load(open(args.census))
    else:
        slots = census()
        if args.census:
            with open(args.census, "w") as f:
                json.dump(slots, f)
    if args.census_only:
        print(json.dumps(slots))
        return
    import torch
    import boojum_amd
    from boojum_amd import pow as W
    if not torch.cuda.is_available():
        raise SystemExit("pow_bench needs a GPU")
    lib = boojum_amd.load()
    line = {"shape": "seed 40 bytes, pow_bits %d, %d seeds" % (args.pow_bits, args.n_seeds),
            "device": torch.cuda.get_device_name(0), "pow_bits": args.pow_bits, "n_seeds": args.n_seeds,
            "peak_lane_slots_per_s": PEAK_LANE_SLOTS}
    for name in HASHERS:
        r = dict(slots[name])
        r.update(run_times(lib, torch, name, args.pow_bits, args.n_seeds))
        r.update(hash_rate(torch, W, name))
        r["slot_floor_ghs"] = PEAK_LANE_SLOTS / r["slots_per_hash"] / 1e9
        r["fraction_of_slot_floor"] = r["rate_ghs"] / r["slot_floor_ghs"]
        line[name] = r
    line["verified"] = True
    print(json.dumps(line))


if __name__ == "__main__":
    main()
