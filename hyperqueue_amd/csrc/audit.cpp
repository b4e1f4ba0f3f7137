// hqaudit::Auditor (audit.h): the one call behind hqtick_resident_check.
#include "audit.h"

#include <cstring>

namespace hqaudit {

#define A_HIP(call)                                                                                       \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) return fail(HQTICK_E_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

int Auditor::run(hipStream_t s, State S, const Totals &t, const RetrHost &retr, const ReqHost &req, hqtick_check_report *out) {
    if (S.have & HAVE_LEDGER) {  // the request tables: [rq_off Q + 1][vent_off NV + 1][ent_res NE][var_nodes NV] u32, [ent_amt NE] u64, [ent_kind NE] u8
        const size_t nq = req.rq_off->size(), nvo = req.vent_off->size(), ne = req.ent_res->size(), nv = nvo - 1;
        const size_t words = nq + nvo + ne + nv, amt_at = (words * 4 + 7) & ~(size_t)7;
        if (!h_req.ensure(amt_at + ne * 9 + 16)) return fail(HQTICK_E_DEVICE, "hipHostMalloc audit staging");
        unsigned char *h = h_req.as<unsigned char>(), *d = h_req.dev<unsigned char>();
        uint32_t *hw = reinterpret_cast<uint32_t *>(h); const uint32_t *dw = reinterpret_cast<const uint32_t *>(d);
        memcpy(hw, req.rq_off->data(), nq * 4); memcpy(hw + nq, req.vent_off->data(), nvo * 4);
        if (ne) memcpy(hw + nq + nvo, req.ent_res->data(), ne * 4);
        for (size_t v = 0; v < nv; v++) hw[nq + nvo + ne + v] = v < req.var_nodes->size() ? (*req.var_nodes)[v] : 0u;
        if (ne) { memcpy(h + amt_at, req.ent_amt->data(), ne * 8); memcpy(h + amt_at + ne * 8, req.ent_kind->data(), ne); }
        Ledger &l = S.ledger;
        l.rq_off = dw; l.ventry_off = dw + nq; l.ent_res = dw + nq + nvo; l.var_nodes = dw + nq + nvo + ne;
        l.ent_amount = reinterpret_cast<const uint64_t *>(d + amt_at); l.ent_kind = d + amt_at + ne * 8;
        l.Q = (uint32_t)nq - 1; l.NV = (uint32_t)nv;
    }
    // the Retracting table is host memory and small: packed into pinned staging [task u64 | target u32 | variant u8 | flags u8] x n, read in place by its kernel
    const uint32_t nr = (uint32_t)retr.task.size();
    S.retr = Retr{nullptr, nullptr, nullptr, nullptr, 0};
    if (nr) {
        if (!h_retr.ensure((size_t)nr * 14 + 16)) return fail(HQTICK_E_DEVICE, "hipHostMalloc audit staging");
        unsigned char *h = h_retr.as<unsigned char>(), *d = h_retr.dev<unsigned char>();
        memcpy(h, retr.task.data(), (size_t)nr * 8);
        memcpy(h + (size_t)nr * 8, retr.target.data(), (size_t)nr * 4);
        memcpy(h + (size_t)nr * 12, retr.variant.data(), nr);
        memcpy(h + (size_t)nr * 13, retr.flags.data(), nr);
        S.retr = Retr{reinterpret_cast<const uint64_t *>(d), reinterpret_cast<const uint32_t *>(d + (size_t)nr * 8), d + (size_t)nr * 12, d + (size_t)nr * 13, nr};
    }
    uint64_t count[HQ_INV_N], first[HQ_INV_N];
    for (uint32_t k = 0; k < HQ_INV_N; k++) { count[k] = 0; first[k] = UINT64_MAX; }
    uint64_t ready_seen = 0, graph_seen = 0, ledger_seen[3] = {0, 0, 0};
    out->kernel_us = 0.0;
    if (wants_ready_pass(S) || wants_graph_pass(S) || wants_ledger_pass(S) || wants_retr_pass(S)) {
        if (!ev0) { A_HIP(hipEventCreate(&ev0)); A_HIP(hipEventCreate(&ev1)); }
        if (!d_out.ensure(OUT_WORDS * 8) || !h_out.ensure(OUT_WORDS * 8)) return fail(HQTICK_E_DEVICE, "hipMalloc audit report");
        if (wants_graph_pass(S) && (S.parts & HQ_CHECK_GRAPH) && !d_cnt.ensure((size_t)S.graph.n_slots * 4 + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc audit scratch");
        LedgerScratch x{nullptr, nullptr, nullptr};
        if (wants_ledger_pass(S) && wants_ledger_part(S)) {
            if (!d_led.ensure(ledger_scratch_bytes(S) + 16)) return fail(HQTICK_E_DEVICE, "hipMalloc audit scratch");
            x.cen_counts = d_led.as<uint32_t>(); x.cen_pf = x.cen_counts + (size_t)S.ledger.W * S.ledger.stride; x.roots = x.cen_pf + (size_t)S.ledger.W * S.ledger.pf_stride;
        }
        unsigned long long *w = d_out.as<unsigned long long>();
        const Out o{w, w + HQ_INV_N, w + 2 * HQ_INV_N};
        A_HIP(hipEventRecord(ev0, s));
        A_HIP(hipMemsetAsync(d_out.p, 0, OUT_WORDS * 8, s));
        A_HIP(hipMemsetAsync(o.first, 0xFF, HQ_INV_N * 8, s));  // UINT64_MAX: nothing found
        A_HIP(launch(S, o, d_cnt.as<uint32_t>(), x, s));
        A_HIP(hipMemcpyAsync(h_out.p, d_out.p, OUT_WORDS * 8, hipMemcpyDeviceToHost, s));
        A_HIP(hipEventRecord(ev1, s));
        A_HIP(hipStreamSynchronize(s));
        const uint64_t *h = h_out.as<uint64_t>();
        for (uint32_t k = 0; k < HQ_INV_N; k++) { count[k] = h[k]; first[k] = h[HQ_INV_N + k]; }
        ready_seen = h[2 * HQ_INV_N]; graph_seen = h[2 * HQ_INV_N + 1];
        for (int k = 0; k < 3; k++) ledger_seen[k] = h[2 * HQ_INV_N + 2 + k];
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) out->kernel_us = (double)ms * 1000.0; else (void)hipGetLastError();
    } else {
        A_HIP(hipStreamSynchronize(s));  // behind every queued delta, like the audited case
    }
    finish_report(S, t, ready_seen, graph_seen, ledger_seen, count, first, out);
    return (int)out->n_failed;
}

void Auditor::release() {
    d_out.release(); d_cnt.release(); d_led.release(); h_out.release(); h_retr.release(); h_req.release();
    if (ev0) hipEventDestroy(ev0);
    if (ev1) hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
}

}  // namespace hqaudit
