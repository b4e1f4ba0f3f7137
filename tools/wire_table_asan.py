"""Runs the resident attribute table of the wire encoder under AddressSanitizer + UBSan (tools/wire_table_asan.cpp: hqwtab::Table on its host backend, a
stand-alone program -- nothing is loaded into python) on random delta sequences and compares what it holds with WireTables.build and the bincode oracle.
    python tools/wire_table_asan.py [--seeds 20]
Every seed runs twice: once with the table sized through hqwire_table_config so that the LAST append fills the row and entry allocations, and the last
add_configs the configuration allocations, to the byte (no growth: an off-by-one in a kernel phase reads or writes past an exact-size heap block), and once
from tiny allocations (every growth path).  Staging blocks are of exact size too; the emulated thread order rotates with the seed.  CPU only."""
import argparse
import os
import random
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def build(exe):
    src = os.path.join(ROOT, "tools", "wire_table_asan.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, src])


def arr(a, dtype=None):
    b = b"" if a is None else np.ascontiguousarray(a, dtype).tobytes()
    return struct.pack("<Q", len(b)) + b


def u64(*v):
    return struct.pack("<%dQ" % len(v), *[x & 0xFFFFFFFFFFFFFFFF for x in v])


class Script:
    """the ops of one run and what python expects back at every dump / encode"""

    def __init__(self):
        self.ops, self.checks = [], []

    def add_configs(self, configs, first):
        some = [c[0] is not None for c in configs]
        off = np.zeros(len(configs) + 1, np.uint64)
        off[1:] = np.cumsum([len(c[1]) for c in configs])
        body = np.frombuffer(b"".join(c[1] for c in configs), np.uint8)
        self.ops.append(u64(1, len(configs)) + arr(some, np.uint8) + arr([c[0][0] if c[0] else 0 for c in configs], np.uint64) +
                        arr([c[0][1] if c[0] else 0 for c in configs], np.uint32) + arr(off) + arr(body) + u64(first))

    def add_tasks(self, batch, expect, order=None, plain=False):
        from hyperqueue_amd import wire

        t = wire.WireTables.build(batch, [])
        ids = t.task_id if order is None else np.array(order, np.uint64)
        blob = t.entry_blob[: int(t.entry_off[-1])]  # exact size: no padding byte
        if plain:  # the NULL forms: instance ids zero, every entry None
            self.ops.append(u64(2, len(ids)) + arr(ids) + arr(t.task_rq) + arr(None) + arr(t.task_priority) + arr(t.task_config) + arr(None) + arr(None) + arr(None) + u64(expect))
        else:
            self.ops.append(u64(2, len(ids)) + arr(ids) + arr(t.task_rq) + arr(t.task_instance) + arr(t.task_priority) + arr(t.task_config) + arr(t.entry_some) +
                            arr(t.entry_off) + arr(blob) + u64(expect))

    def remove(self, ids, hit):
        self.ops.append(u64(3, len(ids)) + arr(ids, np.uint64) + u64(hit, len(ids) - hit))

    def set_instance(self, ids, values, hit):
        self.ops.append(u64(4, len(ids)) + arr(ids, np.uint64) + arr(values, np.uint32) + u64(hit, len(ids) - hit))

    def compact_and_dump(self, attrs, configs):
        self.ops.append(u64(5) + u64(6))
        self.checks.append(("dump", dict(attrs), list(configs)))

    def encode(self, rnd, attrs, configs):
        from hyperqueue_amd import wire
        import wire_cases as wc

        pool = sorted(attrs)
        rnd.shuffle(pool)
        worker_ids = [3, 9, 12]
        records = [[(pool.pop(), 0xFF if k % 3 == 0 else k % 4, 0 if k % 3 == 0 else 1) for k in range(min(len(pool), rnd.randint(0, 50)))] for _ in worker_ids]
        retracts = [[], [77, 78], []]
        mn = [(pool.pop(), [1, 2])] if pool else []
        r = wire.WireRecords.build(worker_ids, records, retracts, mn)
        want = wc.oracle_messages(attrs, configs, worker_ids, records, retracts, mn)
        cap = sum(len(b) for _, b in want)  # exact-fit output buffer
        self.ops.append(u64(7, r.n_workers, r.n_records, r.n_mn, cap) + b"".join(arr(a) for a in r.arrays()))
        self.checks.append(("encode", r, want))

    def blob(self, order, cfg):
        return u64(order, *cfg) + b"".join(self.ops)


def make_script(seed):
    """-> (script, config that the last append / add_configs fills exactly)"""
    import wire_table_cases as tc

    rnd = random.Random(5000 + seed)
    s = Script()
    configs = tc.rand_configs(rnd, rnd.randint(1, 3))
    s.add_configs(configs, 0)
    more = tc.rand_configs(rnd, rnd.randint(1, 3)) + [(None, b"last")]
    s.add_configs(more, len(configs))
    configs += more
    attrs, top, max_rows, max_bytes = {}, (2 << 32) | 500, 0, 0
    nbytes = lambda a: sum(len(v[4] or b"") for v in a.values())
    for op_i in range(rnd.randint(8, 16)):
        live = sorted(attrs)
        op = rnd.choice(["append", "append", "merge", "remove", "inc", "assign", "refuse", "plain"]) if live else "append"
        if op in ("append", "plain"):
            n = rnd.choice([1, 7, tc.TILE - 1, tc.TILE, tc.TILE + 1, rnd.randint(1, 200)])
            ids = sorted(rnd.sample(range(top + 1, top + 1 + 2 * n), n))
            batch = {t: tc.rand_attr(rnd, len(configs), big=(k < 8 and op_i % 3 == 0)) for k, t in enumerate(ids)}
            if op == "plain":
                batch = {t: (v[0], 0, v[2], v[3], None) for t, v in batch.items()}
            s.add_tasks(batch, n, plain=(op == "plain"))
            attrs.update(batch)
            top = ids[-1]
        elif op == "merge":
            ids = sorted({rnd.randrange(live[0] - 50, live[-1]) for _ in range(rnd.choice([1, 5, 60]))} - set(attrs))
            if not ids:
                continue
            batch = {t: tc.rand_attr(rnd, len(configs), big=(op_i % 2 == 0)) for t in ids}
            s.add_tasks(batch, len(ids))
            attrs.update(batch)
        elif op == "refuse":
            bad = {live[len(live) // 2]: (0, 0, 0, 0, b"dup"), live[0] - 7: (0, 0, 0, 0, None)}
            s.add_tasks(bad, -1)                                                  # a live id (merge path)
            s.add_tasks({top + 5: (0, 0, 0, 0, None), top + 6: (0, 0, 0, 0, b"x")}, -1, order=[top + 6, top + 5])  # not ascending (append path)
            s.add_tasks({top + 5: (0, 0, 0, len(configs), None)}, -1)             # configuration index
            max_rows, max_bytes = max(max_rows, len(attrs) + 2), max(max_bytes, nbytes(attrs) + 3)  # (a batch needs its room while it is examined)
        elif op == "remove":
            gone = rnd.sample(live, rnd.choice([1, len(live) // 4 + 1, len(live) // 2 + 1, len(live)]))
            ids = gone + [gone[0], 1, top + 99]
            rnd.shuffle(ids)
            s.remove(ids, len(gone))
            for t in gone:
                del attrs[t]
        elif op == "inc":
            ids = rnd.sample(live, min(len(live), 9))
            ids.append(ids[0])
            s.set_instance(ids + [top + 3], None, len(ids))
            for t in ids:
                v = attrs[t]
                attrs[t] = (v[0], (v[1] + 1) & 0xFFFFFFFF, v[2], v[3], v[4])
        elif op == "assign":
            ids = rnd.sample(live, min(len(live), 9))
            vals = [rnd.randrange(1 << 32) for _ in ids]
            s.set_instance(ids + [1], vals + [5], len(ids))
            for t, x in zip(ids, vals):
                v = attrs[t]
                attrs[t] = (v[0], x, v[2], v[3], v[4])
        max_rows, max_bytes = max(max_rows, len(attrs)), max(max_bytes, nbytes(attrs))
        if attrs and op_i % 2 == 0:
            s.encode(rnd, attrs, configs)
        if op_i % 5 == 4:
            s.compact_and_dump(attrs, configs)
    # the last append: to the byte what the row and entry allocations hold
    r, b = len(attrs), nbytes(attrs)
    n = max(max_rows - r, 0) + rnd.randint(1, 9)
    nb = max(max_bytes - b, 0) + rnd.choice([0, 1, 16, 33])
    ids = list(range(top + 1, top + 1 + n))
    batch = {t: (1, 2, 3, 0, None) for t in ids}
    if nb:
        batch[ids[-1]] = (1, 2, 3, 0, rnd.randbytes(nb))
    s.add_tasks(batch, n)
    attrs.update(batch)
    s.encode(rnd, attrs, configs)
    s.compact_and_dump(attrs, configs)
    exact = (r + n, max(1, b + nb), len(configs), max(1, sum(len(c[1]) for c in configs)))
    return s, exact


def check_output(raw, s, want_growths):
    """-> list of problems"""
    from hyperqueue_amd import wire

    bad, pos = [], 0

    def take():
        nonlocal pos
        n = struct.unpack_from("<Q", raw, pos)[0]
        pos += 8 + n
        return raw[pos - n:pos]

    for kind, *want in s.checks:
        code = struct.unpack_from("<Q", raw, pos)[0]
        pos += 8
        if kind == "dump":
            assert code == 6
            stats = struct.unpack_from("<12Q", raw, pos)
            pos += 96
            got = [take() for _ in range(13)]
            t = wire.WireTables.build(want[0], want[1])
            exp = [np.ascontiguousarray(a).tobytes() for a in t.arrays()]
            exp[7], exp[12] = exp[7][: int(t.entry_off[-1])], exp[12][: int(t.body_off[-1])]
            if got != exp or not (stats[0] == stats[1] == len(want[0])):
                bad.append("copy_out after compact differs from WireTables.build")
            if want_growths is not None and (stats[9] != 0) != want_growths:
                bad.append(f"growths = {stats[9]}")
        else:
            assert code == 7
            r, msgs = want
            S = r.n_workers + r.n_mn
            header, status, off = np.frombuffer(take(), np.uint32), np.frombuffer(take(), np.uint8), np.frombuffer(take(), np.uint64)
            nfrag, frag_end, data = np.frombuffer(take(), np.uint32), np.frombuffer(take(), np.uint64), take()
            res = wire.WireResult(int(header[0]), len(data), status, off, data, nfrag, frag_end)
            if not (header[0] == 0 and (status == 0).all() and res.messages(r) == msgs):
                bad.append("encode on the view differs from the oracle")
    if pos != len(raw):
        bad.append("trailing output")
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=20)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "wire_table_asan")
        build(exe)
        bad = runs = 0
        for seed in range(a.seeds):
            s, exact = make_script(seed)
            for cfg, order, growths in ((exact, seed % 3, False), ((4, 16, 1, 4), (seed + 1) % 3, None)):
                path = os.path.join(d, f"s{seed}_{order}.bin")
                open(path, "wb").write(s.blob(order, cfg))
                p = subprocess.run([exe, path], capture_output=True, text=True)
                runs += 1
                if p.returncode != 0:
                    bad += 1
                    print("SANITIZER / failure", seed, cfg, p.returncode, p.stderr[-2500:])
                    continue
                for why in check_output(open(path + ".out", "rb").read(), s, growths):
                    bad += 1
                    print("MISMATCH", seed, cfg, why)
        print(f"{a.seeds} delta sequences x 2 table sizes ({runs} runs) under ASan+UBSan: {bad} problems")
        return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
