// Sanitizer program for the resident attribute table (csrc/wire_table_core.h): hqwtab::Table on its host backend -- every buffer of the table, every
// staging block and every input array an exact-size heap block -- replays a script of deltas under AddressSanitizer + UBSan.  An out-of-bounds access of a
// kernel phase, which the ctypes tests would survive silently and which would be a memory fault on the GPU, aborts here.  Plain g++, no HIP.  Built and
// driven by tools/wire_table_asan.py; CPU only, test tooling.
//   wire_table_asan <script.bin>  ->  <script.bin>.out
// script: u64 order, 4 x u64 hqwire_table_config, then ops: u64 code, arrays as (u64 byte length, payload):
//   1 add_configs  u64 n, some, secs, nanos, body_off, body, i64 expected return
//   2 add_tasks    u64 n, id, rq, inst (empty = NULL), prio, cfg, some (empty = NULL), off (empty = NULL), blob, i64 expected return
//   3 remove       u64 n, id, i64 expected return, u64 expected unknown
//   4 set_instance u64 n, id, values (empty = NULL), i64 expected return, u64 expected unknown
//   5 compact
//   6 dump         -> out: u64 6, 12 x u64 stats, then the 13 arrays of copy_out as (u64 byte length, payload)
//   7 encode       u64 n_workers, n_records, n_mn, capacity, 10 record arrays -> out: u64 7, header[4], slot_status, slot_off, nfrag, frag_end, bytes (each with its length)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../hyperqueue_amd/csrc/wire_table_core.h"

static const uint8_t *cur, *fin;
static std::vector<void *> blocks;
static uint64_t take_u64() {
    if (cur + 8 > fin) { fprintf(stderr, "script truncated\n"); exit(2); }
    uint64_t v;
    memcpy(&v, cur, 8);
    cur += 8;
    return v;
}
static void *take_array(uint64_t *len = nullptr, bool null_if_empty = false) {
    const uint64_t n = take_u64();
    if (len) *len = n;
    if (cur + n > fin) { fprintf(stderr, "script truncated\n"); exit(2); }
    if (!n && null_if_empty) return nullptr;
    void *p = malloc(n ? n : 1);
    memcpy(p, cur, n);
    cur += n;
    blocks.push_back(p);
    return p;
}
static void free_blocks() {
    for (void *p : blocks) free(p);
    blocks.clear();
}
static FILE *out;
static void put_u64(uint64_t v) { fwrite(&v, 8, 1, out); }
static void put_array(const void *p, uint64_t n) {
    put_u64(n);
    if (n) fwrite(p, 1, n, out);
}
static void expect(int64_t got, int64_t want, const char *what, const hqwtab::Table &t, uint64_t op) {
    if (got == want) return;
    fprintf(stderr, "op %llu %s: returned %lld, expected %lld (%s)\n", (unsigned long long)op, what, (long long)got, (long long)want, t.last_error());
    exit(4);
}

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    fseek(f, 0, SEEK_END);
    const long sz = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> buf(sz);
    if (fread(buf.data(), 1, sz, f) != (size_t)sz) return 2;
    fclose(f);
    cur = buf.data();
    fin = cur + sz;
    out = fopen((std::string(argv[1]) + ".out").c_str(), "wb");
    if (!out) return 2;

    const int order = (int)take_u64();
    hqwire_table_config cfg{};
    cfg.initial_rows = take_u64();
    cfg.initial_blob_bytes = take_u64();
    cfg.initial_configs = take_u64();
    cfg.initial_body_bytes = take_u64();
    {
        hqwtab::Table t(new hqwtab::HostBackend(order), &cfg);
        if (!t.init()) return 3;
        for (uint64_t op = 0; cur < fin; op++) {
            const uint64_t code = take_u64();
            if (code == 1) {
                const uint32_t n = (uint32_t)take_u64();
                const uint8_t *some = (const uint8_t *)take_array();
                const uint64_t *secs = (const uint64_t *)take_array();
                const uint32_t *nanos = (const uint32_t *)take_array();
                const uint64_t *off = (const uint64_t *)take_array();
                const uint8_t *body = (const uint8_t *)take_array();
                expect(t.add_configs(n, some, secs, nanos, off, body), (int64_t)take_u64(), "add_configs", t, op);
            } else if (code == 2) {
                const uint64_t n = take_u64();
                const uint64_t *id = (const uint64_t *)take_array();
                const uint32_t *rq = (const uint32_t *)take_array();
                const uint32_t *inst = (const uint32_t *)take_array(nullptr, true);
                const uint64_t *prio = (const uint64_t *)take_array();
                const uint32_t *cf = (const uint32_t *)take_array();
                const uint8_t *some = (const uint8_t *)take_array(nullptr, true);
                const uint64_t *off = (const uint64_t *)take_array(nullptr, true);
                const uint8_t *blob = (const uint8_t *)take_array();
                expect(t.add_tasks(n, id, rq, inst, prio, cf, some, off, blob), (int64_t)take_u64(), "add_tasks", t, op);
            } else if (code == 3) {
                const uint64_t n = take_u64();
                const uint64_t *id = (const uint64_t *)take_array();
                expect(t.remove_tasks(n, id), (int64_t)take_u64(), "remove_tasks", t, op);
                expect((int64_t)t.last_unknown(), (int64_t)take_u64(), "remove_tasks unknown", t, op);
            } else if (code == 4) {
                const uint64_t n = take_u64();
                const uint64_t *id = (const uint64_t *)take_array();
                const uint32_t *val = (const uint32_t *)take_array(nullptr, true);
                expect(t.set_instance(n, id, val), (int64_t)take_u64(), "set_instance", t, op);
                expect((int64_t)t.last_unknown(), (int64_t)take_u64(), "set_instance unknown", t, op);
            } else if (code == 5) {
                expect(t.compact(), 0, "compact", t, op);
            } else if (code == 6) {
                hqwire_table_stats st{};
                t.stats(&st);
                put_u64(6);
                const uint64_t sv[12] = {st.live_rows, st.physical_rows, st.blob_bytes, st.dead_blob_bytes, st.n_configs, st.body_bytes,
                                         st.appends, st.merges, st.compactions, st.growths, st.hbm_bytes, 0};
                fwrite(sv, 8, 12, out);
                const uint64_t n = st.physical_rows, c = st.n_configs;
                const uint64_t len[13] = {8 * n, 4 * n, 4 * n, 8 * n, 4 * n, n, 8 * (n + 1), st.blob_bytes, c, 8 * c, 4 * c, 8 * (c + 1), st.body_bytes};
                void *p[13];
                for (int i = 0; i < 13; i++) p[i] = malloc(len[i] ? len[i] : 1);  // exact sizes: copy_out must not write past them
                hqwire_tables h{};
                h.task_id = (uint64_t *)p[0]; h.task_rq = (uint32_t *)p[1]; h.task_instance = (uint32_t *)p[2]; h.task_priority = (uint64_t *)p[3];
                h.task_config = (uint32_t *)p[4]; h.entry_some = (uint8_t *)p[5]; h.entry_off = (uint64_t *)p[6]; h.entry_blob = (uint8_t *)p[7];
                h.config_time_some = (uint8_t *)p[8]; h.config_time_secs = (uint64_t *)p[9]; h.config_time_nanos = (uint32_t *)p[10];
                h.body_off = (uint64_t *)p[11]; h.body_blob = (uint8_t *)p[12];
                expect(t.copy_out(&h), 0, "copy_out", t, op);
                for (int i = 0; i < 13; i++) { put_array(p[i], len[i]); free(p[i]); }
            } else if (code == 7) {
                hqwire::Args a{};
                t.view(&a.t);
                a.r.n_workers = (uint32_t)take_u64();
                a.r.n_records = (uint32_t)take_u64();
                a.r.n_mn = (uint32_t)take_u64();
                const uint64_t capacity = take_u64();
                a.r.worker_id = (const uint32_t *)take_array();
                a.r.rec_off = (const uint32_t *)take_array();
                a.r.rec_task = (const uint64_t *)take_array();
                a.r.rec_variant = (const uint8_t *)take_array();
                a.r.rec_kind = (const uint8_t *)take_array();
                a.r.retract_off = (const uint32_t *)take_array();
                a.r.retract_task = (const uint64_t *)take_array();
                a.r.mn_task = (const uint64_t *)take_array();
                a.r.mn_worker_off = (const uint32_t *)take_array();
                a.r.mn_worker = (const uint32_t *)take_array();
                a.n_slots = a.r.n_workers + a.r.n_mn;
                const uint64_t S = a.n_slots, sb = hqwire::scratch_bytes((uint64_t)a.r.n_records + a.r.n_mn, S);
                a.o.bytes = (uint8_t *)malloc(capacity ? capacity : 1);
                a.o.capacity = capacity;
                a.o.slot_off = (uint64_t *)malloc(8 * (2 * S + 1));
                a.o.slot_status = (uint8_t *)malloc(S ? S : 1);
                a.o.header = (uint32_t *)malloc(16);
                a.o.scratch = malloc(sb);
                a.o.scratch_bytes = sb;
                a.o.slot_nfrag = (uint32_t *)malloc(S ? 4 * S : 1);
                a.o.frag_end = (uint64_t *)malloc(S ? 8 * S * HQWIRE_MAX_FRAGMENTS : 1);
                hqwire::bind_scratch(a);
                if (!hqwire::run_on_host(a, order)) return 3;
                const uint64_t total = (uint64_t)a.o.header[2] | (uint64_t)a.o.header[3] << 32;
                put_u64(7);
                put_array(a.o.header, 16);
                put_array(a.o.slot_status, S);
                put_array(a.o.slot_off, 8 * (2 * S + 1));
                put_array(a.o.slot_nfrag, 4 * S);
                put_array(a.o.frag_end, 8 * S * HQWIRE_MAX_FRAGMENTS);
                put_array(a.o.bytes, a.o.header[0] == HQWIRE_OK ? total : 0);
                free(a.o.bytes); free(a.o.slot_off); free(a.o.slot_status); free(a.o.header); free(a.o.scratch); free(a.o.slot_nfrag); free(a.o.frag_end);
            } else {
                fprintf(stderr, "unknown op %llu\n", (unsigned long long)code);
                return 2;
            }
            free_blocks();
        }
    }
    fclose(out);
    return 0;
}
