"""The audit of the resident state (hqtick_resident_check; csrc/audit_core.h) on synthetic tables: one consistent state that holds every structure the audit reads,
one corruption per invariant, and a restatement of every invariant in plain Python / numpy that knows nothing of the C code (`expect`).

Nothing here needs a GPU.  tests/test_audit_core.py runs the states through hqtick_debug_audit_host (the kernels' item functions on host arrays, three thread
orders) and through tools/audit_core_asan.cpp (the same under AddressSanitizer, every table in a heap block of its exact size).

The state: W = 5 workers, R = 3 resources; requests with 1, 2 and 17 variants and a multi-node one (21 variant slots: the count rows are 32 wide); a ledger of
single-node, prefilled and one multi-node entry in 64 buckets, two of its keys at home in the last bucket (the second wraps to bucket 0); a graph with stale
edges, a chain of two runs and a run of 70 edges; a ready column of 300 rows with tombstones; two Retracting entries."""
import copy
import ctypes as C

import numpy as np

from hyperqueue_amd import abi

M64 = (1 << 64) - 1
HT_EMPTY, HT_TOMB = M64, M64 - 1
NONE = 0xFFFFFFFF
TOMB_RQ = 0xFFFFFFFF
MN_VARIANT, PF_VARIANT = 0xFF, 0xFE
SN_FLAG = 1
HAVE_READY, HAVE_GRAPH, HAVE_LEDGER, HAVE_SETTLED, HAVE_TRACKING = 1, 2, 4, 8, 16
RETR_IN_QUEUE, RETR_REDIRECT = 1, 2


def ht_hash(k: int) -> int:
    """the murmur3 finaliser of csrc/graph.hip and csrc/assigned.hip, low 32 bits"""
    k ^= k >> 33; k = (k * 0xFF51AFD7ED558CCD) & M64
    k ^= k >> 33; k = (k * 0xC4CEB9FE1A85EC53) & M64
    k ^= k >> 33
    return k & 0xFFFFFFFF


def ht_insert(keys, mask, k):
    h = ht_hash(k) & mask
    while int(keys[h]) != HT_EMPTY:
        h = (h + 1) & mask
    keys[h] = k
    return h


def ht_find(keys, mask, k):
    """linear probing: the bucket of k, None if an EMPTY bucket comes first"""
    if k >= HT_TOMB:
        return None
    h = ht_hash(k) & mask
    for _ in range(mask + 1):
        if int(keys[h]) == k:
            return h
        if int(keys[h]) == HT_EMPTY:
            return None
        h = (h + 1) & mask
    return None


# ---- the C struct of include/hqtick_debug.h --------------------------------------------------------------------------------------------------------------------
_P = {np.uint64: abi.u64p, np.uint32: abi.u32p, np.uint8: abi.u8p}
FIELDS = [
    ("have", C.c_uint32), ("ready_n", C.c_uint64), ("ready_live", C.c_uint64), ("ready_id", np.uint64), ("ready_rq", np.uint32),
    ("g_slots", C.c_uint32), ("g_runs", C.c_uint32), ("g_edges", C.c_uint32), ("g_free", C.c_uint32), ("g_ht_mask", C.c_uint32), ("g_tasks", C.c_uint64),
    ("g_id", np.uint64), ("g_unfinished", np.uint32), ("g_gen", np.uint32), ("g_head", np.uint32), ("g_ht_key", np.uint64), ("g_ht_val", np.uint32),
    ("g_run_next", np.uint32), ("g_run_off", np.uint32), ("g_run_len", np.uint32), ("g_edge", np.uint32),
    ("l_mask", C.c_uint32), ("l_Q", C.c_uint32), ("l_NV", C.c_uint32), ("l_W", C.c_uint32), ("l_R", C.c_uint32), ("l_stride", C.c_uint32), ("l_pf_stride", C.c_uint32),
    ("l_n_live", C.c_uint64), ("l_mn_live", C.c_uint64), ("l_pf_live", C.c_uint64),
    ("l_key", np.uint64), ("l_worker", np.uint32), ("l_rq", np.uint32), ("l_variant", np.uint8),
    ("l_rq_off", np.uint32), ("l_ventry_off", np.uint32), ("l_ent_res", np.uint32), ("l_var_nodes", np.uint32), ("l_ent_kind", np.uint8), ("l_ent_amount", np.uint64),
    ("l_wid", np.uint32), ("l_total", np.uint64), ("l_free", np.uint64), ("l_counts", np.uint32), ("l_pf", np.uint32), ("l_mn_task", np.uint64), ("l_mn_root", np.uint8),
    ("l_flags", np.uint8),
    ("r_n", C.c_uint32), ("r_task", np.uint64), ("r_target", np.uint32), ("r_variant", np.uint8), ("r_flags", np.uint8),
]


def is_array(t):
    return t in _P


class AuditTablesC(C.Structure):
    _fields_ = [(n, _P[t] if is_array(t) else t) for n, t in FIELDS]


def to_c(st: dict):
    """the state as the C struct (and the arrays it points into, to be kept alive)"""
    c, keep = AuditTablesC(), []
    for n, t in FIELDS:
        if is_array(t):
            a = np.ascontiguousarray(st[n], t)
            keep.append(a)
            setattr(c, n, a.ctypes.data_as(_P[t]) if a.size else None)
        else:
            setattr(c, n, int(st[n]))
    return c, keep


def dump(st: dict) -> bytes:
    """the state for tools/audit_core_asan.cpp: per field of FIELDS, in order, a record [u64 byte count][bytes]; a scalar is one u64"""
    out = bytearray()
    for n, t in FIELDS:
        b = np.ascontiguousarray(st[n], t).tobytes() if is_array(t) else np.uint64(int(st[n])).tobytes()
        out += np.uint64(len(b)).tobytes() + b
    return bytes(out)


# ---- the consistent state -------------------------------------------------------------------------------------------------------------------------------------
WIDS = [3, 7, 8, 20, 21]                      # rows 3 and 4 run the multi-node task
R = 3
NVAR = [1, 2, 17, 1]                          # request 3 is the multi-node one
BIG = 0x9000000000000000                      # twice this wraps 64 bits
TOTAL = [[100_000, 80_000, 0x7000000000000000]] * 5


def _requests():
    rq_off = np.cumsum([0] + NVAR).astype(np.uint32)
    ent = []   # per slot: [(resource, kind, amount)]
    for q, nv in enumerate(NVAR):
        for v in range(nv):
            s = int(rq_off[q]) + v
            if q == 0:
                ent.append([(0, 0, 10_000)])
            elif q == 1:
                ent.append([(0, 0, 5_000), (1, 0, 20_000)] if v == 0 else [(1, 1, 0)])        # variant 1: ALL of resource 1
            elif q == 2:
                ent.append([(2, 0, BIG)] if v == 16 else [(0, 0, 1_000 + s), (1, 0, 100 * (v + 1))])   # variant 16: an amount whose double wraps
            else:
                ent.append([(0, 0, 10_000)])
    ventry_off = np.cumsum([0] + [len(e) for e in ent]).astype(np.uint32)
    flat = [x for e in ent for x in e]
    var_nodes = np.zeros(len(ent), np.uint32); var_nodes[int(rq_off[3])] = 2
    return dict(l_rq_off=rq_off, l_ventry_off=ventry_off, l_ent_res=np.asarray([x[0] for x in flat], np.uint32), l_ent_kind=np.asarray([x[1] for x in flat], np.uint8),
                l_ent_amount=np.asarray([x[2] for x in flat], np.uint64), l_var_nodes=var_nodes, l_Q=len(NVAR), l_NV=len(ent))


def _last_bucket_ids(mask, n, lo):
    out, k = [], lo
    while len(out) < n:
        if ht_hash(k) & mask == mask:
            out.append(k)
        k += 1
    return out


class _GraphBuilder:
    """slots, generations, run chains and the hash table as csrc/graph.hip leaves them (one run per producer and add call; a removed task's slot is recycled)"""

    def __init__(self, ht_cap):
        self.id, self.unf, self.gen, self.head = [], [], [], []
        self.free, self.slot_of = [], {}
        self.run_next, self.run_off, self.run_len, self.edge = [], [], [], []
        self.ht_key = np.full(ht_cap, HT_EMPTY, np.uint64); self.ht_val = np.zeros(ht_cap, np.uint32); self.mask = ht_cap - 1

    def add(self, ids, deps_of):
        """one batch: ids in submission order; deps_of(id) -> producer ids (kept if they are in the graph and not of this batch)"""
        before = dict(self.slot_of)
        runs = {}
        for i in ids:
            if self.free:
                sl = self.free.pop()
            else:
                sl = len(self.id); self.id.append(0); self.unf.append(0); self.gen.append(0); self.head.append(NONE)
            self.id[sl], self.unf[sl], self.head[sl] = i, 0, NONE
            self.slot_of[i] = sl
            p = ht_insert(self.ht_key, self.mask, i); self.ht_val[p] = sl
            for d in deps_of(i):
                if d in before:
                    self.unf[sl] += 1
                    runs.setdefault(d, []).append((sl, self.gen[sl]))
        for d, es in runs.items():
            ps = before[d]
            self.run_next.append(self.head[ps]); self.run_off.append(len(self.edge)); self.run_len.append(len(es))
            self.head[ps] = len(self.run_next) - 1
            self.edge += es

    def remove(self, i):
        """the task leaves: key to a tombstone, generation bumped, slot recycled, its runs dropped; its consumers keep their counters (a caller's business)"""
        sl = self.slot_of.pop(i)
        self.ht_key[ht_find(self.ht_key, self.mask, i)] = HT_TOMB
        self.unf[sl] = NONE; self.gen[sl] += 1; self.head[sl] = NONE; self.free.append(sl)

    def finish(self, i):
        """task_finished: the consumers' counters drop, then the task leaves"""
        sl = self.slot_of[i]
        r = self.head[sl]
        while r != NONE:
            for e in range(self.run_off[r], self.run_off[r] + self.run_len[r]):
                c, g = self.edge[e]
                if self.gen[c] == g:
                    self.unf[c] -= 1
            r = self.run_next[r]
        self.remove(i)


def consistent() -> dict:
    st = {}
    st.update(_requests())
    W, mask = len(WIDS), 63
    stride, pf_stride = 32, 16                     # row_stride(21 slots), row_stride(4 requests)
    rq_off = st["l_rq_off"]
    # ---- ledger entries: (id, worker id, rq, variant)
    wrap = _last_bucket_ids(mask, 2, 5000)
    sn = [(101, 3, 0, 0), (102, 3, 0, 0), (103, 3, 1, 0), (104, 7, 1, 1), (105, 7, 2, 3), (106, 7, 2, 16), (107, 7, 2, 16), (108, 8, 2, 0), (109, 8, 2, 15),
          (wrap[0], 8, 0, 0), (wrap[1], 3, 2, 7), (110, 7, 0, 0)]
    mn = [(201, 20, 3, MN_VARIANT)]                # root on worker 20 (row 3), also on worker 21 (row 4)
    pf = [(301, 3, 0, PF_VARIANT), (302, 3, 0, PF_VARIANT), (303, 8, 2, PF_VARIANT)]
    key = np.full(mask + 1, HT_EMPTY, np.uint64); worker = np.zeros(mask + 1, np.uint32); rq = np.zeros(mask + 1, np.uint32); var = np.zeros(mask + 1, np.uint8)
    ht_insert(key, mask, 999); key[ht_find(key, mask, 999)] = HT_TOMB   # a released task's tombstone
    for (i, w, q, v) in sn + mn + pf:
        b = ht_insert(key, mask, i); worker[b], rq[b], var[b] = w, q, v
    assert ht_find(key, mask, wrap[1]) == 0 and ht_find(key, mask, wrap[0]) == mask
    counts = np.zeros((W, stride), np.uint32); pfc = np.zeros((W, pf_stride), np.uint32)
    for (i, w, q, v) in sn:
        counts[WIDS.index(w), int(rq_off[q]) + v] += 1
    for (i, w, q, v) in pf:
        pfc[WIDS.index(w), q] += 1
    flags = np.asarray([1, 1, 1 | 2, 0, 0], np.uint8)   # row 2 is stopping as well; rows 3, 4 hold the multi-node task
    total = np.asarray(TOTAL, np.uint64)
    free = total.copy()
    for w in range(W):
        for r in range(R):
            free[w, r] = _free_of(st, counts, total, w, r, stride)
    free[3] = [1, 2, 3]; free[4] = [4, 5, 6]          # rows without the SN bit: whatever they held when the task came
    mn_task = np.full(W, HT_EMPTY, np.uint64); mn_root = np.zeros(W, np.uint8)
    mn_task[3] = mn_task[4] = 201; mn_root[3] = 1
    st.update(l_mask=mask, l_W=W, l_R=R, l_stride=stride, l_pf_stride=pf_stride, l_n_live=len(sn), l_mn_live=len(mn), l_pf_live=len(pf), l_key=key, l_worker=worker, l_rq=rq,
              l_variant=var, l_wid=np.asarray(WIDS, np.uint32), l_total=total.ravel(), l_free=free.ravel(), l_counts=counts.ravel(), l_pf=pfc.ravel(), l_mn_task=mn_task,
              l_mn_root=mn_root, l_flags=flags)
    ledger_ids = [e[0] for e in sn + mn + pf]
    # ---- ready column: 300 rows; every 9th a tombstone of a task that went into the ledger or was cancelled
    ready_ids = list(range(10_000, 10_000 + 3 * 300, 3))
    spare = sorted(ledger_ids)                        # consumed tasks keep their ids as tombstones: the ledger's ids sit in the column, dead
    col = sorted(ready_ids[: 300 - len(spare)] + spare)
    rqc = np.asarray([(i // 3) % 3 for i in col], np.uint32)
    for k, i in enumerate(col):
        if i in spare or k % 9 == 4:
            rqc[k] = TOMB_RQ
    live_ready = [i for k, i in enumerate(col) if rqc[k] != TOMB_RQ]
    st.update(ready_n=len(col), ready_live=len(live_ready), ready_id=np.asarray(col, np.uint64), ready_rq=rqc)
    # ---- graph: every ready and every ledger task with counter 0, and waiting tasks behind them
    g = _GraphBuilder(1024)
    g.add(live_ready + ledger_ids, lambda i: [])
    P1, P2, P3 = ledger_ids[0], ledger_ids[1], live_ready[0]
    g.add(list(range(400, 440)), lambda i: [P1] if i % 2 else [P1, P2])         # 40 waiting tasks; P1 has a run of 40
    for i in (401, 403, 405, 402):
        g.remove(i)                                                               # their edges in P1's / P2's runs go stale
    g.add([500, 501, 502, 503], lambda i: [P2, P3])                             # heirs move into the freed slots and wait for P2 and P3: a second run on P2
    g.add(list(range(600, 670)), lambda i: [P3])                                # one run of 70 edges: more than a wavefront
    g.add([700], lambda i: [600, 669, 500])
    g.add([9000], lambda i: []); g.finish(9000)                                  # a slot on the free stack at the end
    assert len(g.free) == 1
    n = len(g.id)
    st.update(g_slots=n, g_runs=len(g.run_next), g_edges=len(g.edge), g_free=len(g.free), g_ht_mask=g.mask, g_tasks=len(g.slot_of), g_id=np.asarray(g.id, np.uint64),
              g_unfinished=np.asarray(g.unf, np.uint32), g_gen=np.asarray(g.gen, np.uint32), g_head=np.asarray(g.head, np.uint32), g_ht_key=g.ht_key, g_ht_val=g.ht_val,
              g_run_next=np.asarray(g.run_next, np.uint32), g_run_off=np.asarray(g.run_off, np.uint32), g_run_len=np.asarray(g.run_len, np.uint32),
              g_edge=np.asarray(g.edge, np.uint32).ravel())
    # ---- Retracting: one back in its queue, one redirected to worker 7 with variant 3 (ledger entry 105)
    st.update(r_n=2, r_task=np.asarray([live_ready[5], 105], np.uint64), r_target=np.asarray([NONE, 7], np.uint32), r_variant=np.asarray([0, 3], np.uint8),
              r_flags=np.asarray([RETR_IN_QUEUE, RETR_REDIRECT], np.uint8))
    st["have"] = HAVE_READY | HAVE_GRAPH | HAVE_LEDGER | HAVE_SETTLED | HAVE_TRACKING
    st["_names"] = dict(wrap=wrap, live_ready=live_ready, ledger_ids=ledger_ids, P3=P3, fan=list(range(600, 670)))
    return st


def _free_of(st, counts, total, w, r, stride):
    """resources.clone() then remove(rq) per assigned task (workerload.rs:156-166), from the counts: ALL leaves 0, AMOUNT subtracts, saturating at 0"""
    all_, s_ = False, 0
    for s in range(min(int(st["l_NV"]), stride)):
        c = int(counts[w, s])
        if not c:
            continue
        for e in range(int(st["l_ventry_off"][s]), int(st["l_ventry_off"][s + 1])):
            if int(st["l_ent_res"][e]) != r:
                continue
            if int(st["l_ent_kind"][e]) == 1:
                all_ = True
            else:
                s_ = min(M64, s_ + min(M64, c * int(st["l_ent_amount"][e])))   # Python integers do not wrap: min() is the saturation
    t = int(total[w, r])
    return 0 if all_ else max(0, t - s_)


# ---- the invariants, restated ----------------------------------------------------------------------------------------------------------------------------------
def expect(st: dict, parts: int):
    """(checked, {invariant name: (count, first)}) as include/hqtick.h defines them, from the arrays alone"""
    have = int(st["have"])
    rd, gr_res, lg = bool(have & HAVE_READY), bool(have & HAVE_GRAPH), bool(have & HAVE_LEDGER)
    gr = gr_res and int(st["g_tasks"]) != 0
    settled, tracking = bool(have & HAVE_SETTLED), bool(have & HAVE_TRACKING)
    checked = 0
    if rd: checked |= abi.HQ_CHECK_READY
    if lg: checked |= abi.HQ_CHECK_LEDGER
    if gr_res: checked |= abi.HQ_CHECK_GRAPH
    if (rd and lg) or (rd and gr) or (int(st["r_n"]) and (rd or lg)): checked |= abi.HQ_CHECK_CROSS
    if gr and (rd or lg): checked |= abi.HQ_CHECK_STRICT
    checked &= parts
    hits = {}

    def hit(name, key):
        hits.setdefault(name, []).append(int(key))

    rid, rrq = [int(x) for x in st["ready_id"]], [int(x) for x in st["ready_rq"]]
    lkey, lmask = st["l_key"], int(st["l_mask"])
    gid, gunf = [int(x) for x in st["g_id"]], [int(x) for x in st["g_unfinished"]]
    n_slots = int(st["g_slots"])

    def g_slot(i):
        p = ht_find(st["g_ht_key"], int(st["g_ht_mask"]), i)
        if p is None:
            return None
        sl = int(st["g_ht_val"][p])
        return sl if sl < n_slots and gunf[sl] != NONE else None

    def in_ledger(i):
        return lg and ht_find(lkey, lmask, i) is not None

    live_ready_ids = {i for i, q in zip(rid, rrq) if q != TOMB_RQ}

    def ready_is_live(i):   # by membership, not by the library's binary search
        return i in live_ready_ids

    if rd:
        live = 0
        for k, i in enumerate(rid):
            if checked & abi.HQ_CHECK_READY and k and rid[k - 1] >= i:
                hit("HQ_INV_READY_ORDER", i)
            if rrq[k] == TOMB_RQ:
                continue
            live += 1
            if checked & abi.HQ_CHECK_CROSS and in_ledger(i):
                hit("HQ_INV_X_READY_ASSIGNED", i)
            if gr:
                sl = g_slot(i)
                if sl is None:
                    if checked & abi.HQ_CHECK_STRICT: hit("HQ_INV_S_READY_UNKNOWN", i)
                elif checked & abi.HQ_CHECK_CROSS and gunf[sl] != 0:
                    hit("HQ_INV_X_READY_WAITING", i)
        if checked & abi.HQ_CHECK_READY and live != int(st["ready_live"]):
            hit("HQ_INV_READY_COUNT", live)
    if gr_res and checked & (abi.HQ_CHECK_GRAPH | abi.HQ_CHECK_STRICT):
        live_slots = [s for s in range(n_slots) if gunf[s] != NONE]
        edges_in = [0] * n_slots
        for s in live_slots:
            r, steps = int(st["g_head"][s]), 0
            while r != NONE and r < int(st["g_runs"]) and steps < int(st["g_runs"]):
                off, ln = int(st["g_run_off"][r]), int(st["g_run_len"][r])
                for e in range(off, off + ln):
                    c, gn = int(st["g_edge"][2 * e]), int(st["g_edge"][2 * e + 1])
                    if c < n_slots and int(st["g_gen"][c]) == gn:
                        edges_in[c] += 1
                r, steps = int(st["g_run_next"][r]), steps + 1
        for s in live_slots:
            if checked & abi.HQ_CHECK_GRAPH:
                p = ht_find(st["g_ht_key"], int(st["g_ht_mask"]), gid[s])
                if p is None or int(st["g_ht_val"][p]) != s:
                    hit("HQ_INV_GRAPH_HASH", gid[s])
                if gunf[s] != edges_in[s]:
                    hit("HQ_INV_GRAPH_COUNTER", gid[s])
            if checked & abi.HQ_CHECK_STRICT and rd and lg and tracking and gunf[s] == 0 and not ready_is_live(gid[s]) and not in_ledger(gid[s]):
                hit("HQ_INV_S_RELEASED_NOWHERE", gid[s])
        if checked & abi.HQ_CHECK_GRAPH and (len(live_slots) != int(st["g_tasks"]) or len(live_slots) + int(st["g_free"]) != n_slots):
            hit("HQ_INV_GRAPH_TOTALS", len(live_slots))
    if lg and checked & (abi.HQ_CHECK_LEDGER | abi.HQ_CHECK_STRICT):
        W, stride, pfs, Q, NV = int(st["l_W"]), int(st["l_stride"]), int(st["l_pf_stride"]), int(st["l_Q"]), int(st["l_NV"])
        wid = [int(x) for x in st["l_wid"]]
        rq_off = [int(x) for x in st["l_rq_off"]]
        counts = np.asarray(st["l_counts"], np.uint32).reshape(W, stride); pfc = np.asarray(st["l_pf"], np.uint32).reshape(W, pfs)
        cen = np.zeros((W, stride), np.int64); cen_pf = np.zeros((W, pfs), np.int64); census = [0, 0, 0]
        roots = {}
        part = bool(checked & abi.HQ_CHECK_LEDGER)
        if part:
            for w in range(W):
                t, root = int(st["l_mn_task"][w]), int(st["l_mn_root"][w])
                if t == HT_EMPTY:
                    if root: hit("HQ_INV_LEDGER_MN", wid[w])
                    continue
                b = ht_find(lkey, lmask, t)
                bad = b is None or int(st["l_variant"][b]) != MN_VARIANT
                if not bad and root:
                    if int(st["l_worker"][b]) == wid[w]: roots[b] = roots.get(b, 0) + 1
                    else: bad = True
                bad = bad or bool(int(st["l_flags"][w]) & SN_FLAG) or bool(counts[w].any())
                if bad: hit("HQ_INV_LEDGER_MN", t)
        for b in range(lmask + 1):
            k = int(lkey[b])
            if k >= HT_TOMB:
                continue
            v = int(st["l_variant"][b])
            cls = 1 if v == MN_VARIANT else 2 if v == PF_VARIANT else 0
            census[cls] += 1
            if checked & abi.HQ_CHECK_STRICT and gr:
                sl = g_slot(k)
                if sl is None or gunf[sl] != 0: hit("HQ_INV_S_ASSIGNED_WAITING", k)
            if not part:
                continue
            if ht_find(lkey, lmask, k) != b: hit("HQ_INV_LEDGER_HASH", k)
            w, q = int(st["l_worker"][b]), int(st["l_rq"][b])
            ok = w in wid and q < Q
            if ok:
                row, s0, nvar = wid.index(w), rq_off[q], rq_off[q + 1] - rq_off[q]
                if cls == 0:
                    ok = v < nvar and s0 + v < stride
                    if ok: cen[row, s0 + v] += 1
                elif cls == 1:
                    ok = s0 < NV and int(st["l_var_nodes"][s0]) > 0
                    if ok and roots.get(b, 0) != 1: hit("HQ_INV_LEDGER_MN", k)
                else:
                    ok = tracking and q < pfs
                    if ok: cen_pf[row, q] += 1
            if not ok: hit("HQ_INV_LEDGER_ENTRY", k)
        if part:
            want = (int(st["l_n_live"]), int(st["l_mn_live"]), int(st["l_pf_live"]) if tracking else 0)
            if tuple(census) != want:
                f = lambda x: min(x, (1 << 21) - 1)
                hit("HQ_INV_LEDGER_TOTALS", f(census[0]) | f(census[1]) << 21 | f(census[2]) << 42)
            total = np.asarray(st["l_total"], np.uint64).reshape(W, int(st["l_R"])); free = np.asarray(st["l_free"], np.uint64).reshape(W, int(st["l_R"]))
            for w in range(W):
                for s in range(stride):
                    if int(counts[w, s]) != int(cen[w, s]): hit("HQ_INV_LEDGER_COUNTS", wid[w] << 32 | s)
                for q in range(pfs if tracking else 0):
                    if int(pfc[w, q]) != int(cen_pf[w, q]): hit("HQ_INV_LEDGER_PREFILLED", wid[w] << 32 | q)
                if int(st["l_flags"][w]) & SN_FLAG:
                    for r in range(int(st["l_R"])):
                        if int(free[w, r]) != _free_of(st, counts, total, w, r, stride): hit("HQ_INV_LEDGER_FREE", wid[w] << 32 | r)
    if checked & abi.HQ_CHECK_CROSS:
        for j in range(int(st["r_n"])):
            i, f = int(st["r_task"][j]), int(st["r_flags"][j])
            bad = bool(f & RETR_IN_QUEUE) and rd and not ready_is_live(i)
            if f & RETR_REDIRECT and lg and settled:
                b = ht_find(lkey, lmask, i)
                bad = bad or b is None or int(st["l_worker"][b]) != int(st["r_target"][j]) or int(st["l_variant"][b]) != int(st["r_variant"][j]) or int(st["l_variant"][b]) >= PF_VARIANT
            if bad: hit("HQ_INV_X_RETRACTING", i)
    return checked, {n: (len(v), min(v)) for n, v in hits.items()}


# ---- one corruption per invariant -------------------------------------------------------------------------------------------------------------------------------
STRICT_ALL = abi.HQ_CHECK_ALL | abi.HQ_CHECK_STRICT


def _slot(st, i):
    return int(st["g_ht_val"][ht_find(st["g_ht_key"], int(st["g_ht_mask"]), i)])


def _bucket(st, i):
    return ht_find(st["l_key"], int(st["l_mask"]), i)


def _row(st, i):
    return [int(x) for x in st["ready_id"]].index(i)


def _c_ready_order_256(st): st["ready_id"][256] = st["ready_id"][255]
def _c_ready_order_last(st): st["ready_id"][-1] = 0
def _c_ready_count(st): st["ready_live"] += 1
def _c_ledger_hash_wrap(st): st["l_key"][int(st["l_mask"])] = HT_EMPTY          # the key at home in the last bucket goes: the one that wrapped to bucket 0 is cut off
def _c_ledger_entry(st): st["l_variant"][_bucket(st, 103)] = 5                     # request 1 has two variants
def _c_ledger_totals(st): st["l_n_live"] += 1
def _c_ledger_counts(st): st["l_counts"][0 * 32 + 0] += 1                          # one more task of (request 0, variant 0) on worker 3 than the table holds
def _c_ledger_prefilled(st): st["l_pf"][2 * 16 + 2] += 1
def _c_ledger_free(st): st["l_free"][1 * 3 + 0] += 1
def _c_ledger_free_wrapped(st): st["l_free"][1 * 3 + 2] = (0x7000000000000000 - 2 * BIG) & M64   # what a wrapping product would leave of resource 2 on worker 7
def _c_ledger_mn(st): st["l_mn_root"][3] = 0
def _c_graph_hash(st): st["g_ht_val"][ht_find(st["g_ht_key"], int(st["g_ht_mask"]), 410)] = _slot(st, 412)
def _c_graph_totals(st): st["g_free"] += 1
def _c_graph_counter_fan(st): st["g_unfinished"][_slot(st, 668)] += 1             # edge 69 of the run of 70
def _c_x_ready_assigned(st): st["ready_rq"][_row(st, 108)] = 0                     # a consumed task's tombstone comes back to life
def _c_x_ready_waiting(st): st["g_unfinished"][_slot(st, st["_names"]["live_ready"][7])] = 1
def _c_x_retracting(st): st["r_task"][0] = st["ready_id"][4]                       # row 4 is a tombstone
def _c_x_retracting_redirect(st): st["r_variant"][1] = 4
def _c_s_ready_unknown(st): st["g_ht_key"][ht_find(st["g_ht_key"], int(st["g_ht_mask"]), st["_names"]["live_ready"][9])] = HT_TOMB
def _c_s_assigned_waiting(st): st["g_unfinished"][_slot(st, 109)] = 2
def _c_s_released_nowhere(st): st["ready_rq"][_row(st, st["_names"]["live_ready"][11])] = TOMB_RQ


# name -> (corruption, parts, the invariant it is about, the others it logically implies)
CASES = {
    "ready_order_256": (_c_ready_order_256, abi.HQ_CHECK_ALL, "HQ_INV_READY_ORDER", ()),
    "ready_order_last": (_c_ready_order_last, abi.HQ_CHECK_ALL, "HQ_INV_READY_ORDER", ()),
    "ready_count": (_c_ready_count, abi.HQ_CHECK_ALL, "HQ_INV_READY_COUNT", ()),
    # the entry that went is missing from the census (totals) and from its (row, slot) count
    "ledger_hash_wrap": (_c_ledger_hash_wrap, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_HASH", ("HQ_INV_LEDGER_TOTALS", "HQ_INV_LEDGER_COUNTS")),
    "ledger_entry": (_c_ledger_entry, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_ENTRY", ("HQ_INV_LEDGER_COUNTS",)),   # an invalid entry is counted in no slot
    "ledger_totals": (_c_ledger_totals, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_TOTALS", ()),
    "ledger_counts": (_c_ledger_counts, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_COUNTS", ("HQ_INV_LEDGER_FREE",)),  # the free row follows from the count table
    "ledger_prefilled": (_c_ledger_prefilled, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_PREFILLED", ()),
    "ledger_free": (_c_ledger_free, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_FREE", ()),
    "ledger_free_wrapped": (_c_ledger_free_wrapped, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_FREE", ()),
    "ledger_mn": (_c_ledger_mn, abi.HQ_CHECK_ALL, "HQ_INV_LEDGER_MN", ()),
    "graph_hash": (_c_graph_hash, abi.HQ_CHECK_ALL, "HQ_INV_GRAPH_HASH", ()),
    "graph_totals": (_c_graph_totals, abi.HQ_CHECK_ALL, "HQ_INV_GRAPH_TOTALS", ()),
    "graph_counter_fan": (_c_graph_counter_fan, abi.HQ_CHECK_ALL, "HQ_INV_GRAPH_COUNTER", ()),
    "x_ready_assigned": (_c_x_ready_assigned, abi.HQ_CHECK_ALL, "HQ_INV_X_READY_ASSIGNED", ("HQ_INV_READY_COUNT",)),   # one more live row than the host counts
    "x_ready_waiting": (_c_x_ready_waiting, abi.HQ_CHECK_ALL, "HQ_INV_X_READY_WAITING", ("HQ_INV_GRAPH_COUNTER",)),   # a counter of 1 with no edge behind it
    "x_retracting": (_c_x_retracting, abi.HQ_CHECK_ALL, "HQ_INV_X_RETRACTING", ()),
    "x_retracting_redirect": (_c_x_retracting_redirect, abi.HQ_CHECK_ALL, "HQ_INV_X_RETRACTING", ()),
    "s_ready_unknown": (_c_s_ready_unknown, STRICT_ALL, "HQ_INV_S_READY_UNKNOWN", ("HQ_INV_GRAPH_HASH",)),             # the slot is live and no longer found
    "s_assigned_waiting": (_c_s_assigned_waiting, STRICT_ALL, "HQ_INV_S_ASSIGNED_WAITING", ("HQ_INV_GRAPH_COUNTER",)),
    "s_released_nowhere": (_c_s_released_nowhere, STRICT_ALL, "HQ_INV_S_RELEASED_NOWHERE", ("HQ_INV_READY_COUNT",)),
}


def corrupted(name: str) -> dict:
    st = copy.deepcopy(consistent())
    CASES[name][0](st)
    return st
