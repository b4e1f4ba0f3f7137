// The audit's item functions (csrc/audit_core.h: what the kernels of csrc/audit.hip run per row, slot, bucket and entry) under AddressSanitizer and UBSan, on
// the states of tests/audit_cases.py.  Stand-alone: g++ -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/audit_core_asan.cpp.
//
//   audit_core_asan STATE_FILE PARTS
//
// STATE_FILE is tests/audit_cases.py's dump(): per field of hqtick_debug_audit_tables, in declaration order, a record [u64 byte count][bytes]; a scalar field is
// one u64.  Every table goes into a heap block of EXACTLY its size, so that a read one element past any of them is a finding.  Runs the host backend in the
// three thread orders and prints, per order, `order K checked C n_failed F` and one line `INV count first` per violated invariant.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../hyperqueue_amd/csrc/audit_core.h"

namespace {

struct Reader {
    FILE *f;
    std::vector<void *> blocks;
    uint64_t scalar() {
        uint64_t n = 0, v = 0;
        if (fread(&n, 8, 1, f) != 1 || n != 8 || fread(&v, 8, 1, f) != 1) { fprintf(stderr, "bad scalar record\n"); exit(2); }
        return v;
    }
    template <typename T> const T *array() {
        uint64_t n = 0;
        if (fread(&n, 8, 1, f) != 1) { fprintf(stderr, "bad array record\n"); exit(2); }
        if (n == 0) return nullptr;
        void *p = malloc(n);  // exact size
        if (!p || fread(p, 1, n, f) != n) { fprintf(stderr, "short array record\n"); exit(2); }
        blocks.push_back(p);
        return static_cast<const T *>(p);
    }
    ~Reader() { for (void *p : blocks) free(p); }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s STATE_FILE PARTS\n", argv[0]); return 2; }
    FILE *f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    Reader rd{f, {}};
    hqaudit::State S{};
    hqaudit::Totals t{};
    S.parts = (uint32_t)strtoul(argv[2], nullptr, 0);
    S.have = (uint32_t)rd.scalar();
    S.ready.n = rd.scalar(); t.ready_live = rd.scalar(); S.ready.id = rd.array<uint64_t>(); S.ready.rq = rd.array<uint32_t>();
    hqaudit::Graph &g = S.graph;
    g.n_slots = (uint32_t)rd.scalar(); g.n_runs = (uint32_t)rd.scalar(); g.n_edges = (uint32_t)rd.scalar(); t.graph_free = rd.scalar(); g.ht_mask = (uint32_t)rd.scalar();
    g.n_tasks = rd.scalar(); t.graph_tasks = g.n_tasks; t.graph_slots = g.n_slots;
    g.id = rd.array<uint64_t>(); g.unfinished = rd.array<uint32_t>(); g.gen = rd.array<uint32_t>(); g.head = rd.array<uint32_t>(); g.ht_key = rd.array<uint64_t>();
    g.ht_val = rd.array<uint32_t>(); g.run_next = rd.array<uint32_t>(); g.run_off = rd.array<uint32_t>(); g.run_len = rd.array<uint32_t>(); g.edge = rd.array<uint32_t>();
    hqaudit::Ledger &l = S.ledger;
    l.mask = (uint32_t)rd.scalar(); l.Q = (uint32_t)rd.scalar(); l.NV = (uint32_t)rd.scalar(); l.W = (uint32_t)rd.scalar(); l.R = (uint32_t)rd.scalar();
    l.stride = (uint32_t)rd.scalar(); l.pf_stride = (uint32_t)rd.scalar(); l.n_live = rd.scalar(); l.mn_live = rd.scalar(); l.pf_live = rd.scalar();
    l.key = rd.array<uint64_t>(); l.worker = rd.array<uint32_t>(); l.rq = rd.array<uint32_t>(); l.variant = rd.array<uint8_t>();
    l.rq_off = rd.array<uint32_t>(); l.ventry_off = rd.array<uint32_t>(); l.ent_res = rd.array<uint32_t>(); l.var_nodes = rd.array<uint32_t>();
    l.ent_kind = rd.array<uint8_t>(); l.ent_amount = rd.array<uint64_t>();
    l.wid = rd.array<uint32_t>(); l.total = rd.array<uint64_t>(); l.free_ = rd.array<uint64_t>(); l.counts = rd.array<uint32_t>(); l.pf = rd.array<uint32_t>();
    l.mn_task = rd.array<uint64_t>(); l.mn_root = rd.array<uint8_t>(); l.flags = rd.array<uint8_t>();
    S.retr.n = (uint32_t)rd.scalar();
    S.retr.task = rd.array<uint64_t>(); S.retr.target = rd.array<uint32_t>(); S.retr.variant = rd.array<uint8_t>(); S.retr.flags = rd.array<uint8_t>();
    fclose(f);
    for (int order = 0; order < 3; order++) {
        hqtick_check_report rep;
        hqaudit::run_host(S, t, order, &rep);
        printf("order %d checked %u n_failed %u\n", order, rep.checked, rep.n_failed);
        for (uint32_t k = 0; k < HQ_INV_N; k++)
            if (rep.count[k]) printf("%u %llu %llu\n", k, (unsigned long long)rep.count[k], (unsigned long long)rep.first[k]);
    }
    return 0;
}
