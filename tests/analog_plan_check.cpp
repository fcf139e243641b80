// Host driver of the analog launch plan (scikit-downscale_amd/csrc/sd_analog_plan.h) for tests/test_analog_plan.py: reads one
// call per line on stdin and prints its plan.
//   in:  op T F C Tq k kind has_thresh neighbors has_sample ld ld_q ld_out lds_max cu_count
//        has_xs has_yx has_ybar has_ps has_pq has_rx
//        no_slab heap no_tile reg_prefix no_runs runs_always readlane slab_classes prune_at ablate  cc
//        (op: 0 fit, 1 PureAnalog predict, 2 AnalogRegression predict, 3 fit + predict; cc: cells of the chunk to list)
//   out: "error <code> <message>", or "plan key=value ..." followed by one line "<launch> <gx> <gy> <gz> <block> <lds>" per geometry
//        function of analog_launches that applies to the operation (whether a launch runs is in the plan's decisions); then "end".
//   A line "sweep <lds_max>" prints "w <T> <sort2_width> <sorted>" for T = 1 .. 20 480 (one-feature fit of 1 000 cells).
#include <cstdio>
#include <iostream>
#include <string>

#include "sd_analog_plan.h"

static void put(const char* launch, const AnalogLaunch& L) {
    printf("%s %lld %lld %lld %d %zu\n", launch, (long long)L.gx, (long long)L.gy, (long long)L.gz, L.block, L.lds);
}

int main() {
    std::string word;
    while (std::cin >> word) {
        AnalogCall c;
        AnalogDevSwitches d;
        if (word == "sweep") {
            std::cin >> c.lds_max;
            c.F = 1, c.C = c.ld = 1000, c.cu_count = 256;
            for (c.T = 1; c.T <= 20480; ++c.T) printf("w %lld %d %d\n", (long long)c.T, sdan::sort2_width(c.T, c.lds_max), analog_plan(c, d).sorted ? 1 : 0);
            printf("end\n");
            continue;
        }
        int op = std::stoi(word), call_flags[3], state[6], sw[7];
        int64_t cc = 0;
        std::cin >> c.T >> c.F >> c.C >> c.Tq >> c.k >> c.kind;
        for (int& f : call_flags) std::cin >> f;
        std::cin >> c.ld >> c.ld_q >> c.ld_out >> c.lds_max >> c.cu_count;
        for (int& f : state) std::cin >> f;
        for (int& f : sw) std::cin >> f;
        std::cin >> d.slab_classes >> d.prune_at >> d.ablate >> cc;
        c.op = (AnalogOp)op;
        c.has_thresh = call_flags[0] != 0, c.neighbors = call_flags[1] != 0, c.has_sample = call_flags[2] != 0;
        c.has_xs = state[0] != 0, c.has_yx = state[1] != 0, c.has_ybar = state[2] != 0, c.has_ps = state[3] != 0, c.has_pq = state[4] != 0,
        c.has_rx = state[5] != 0;
        d.no_slab = sw[0] != 0, d.heap = sw[1] != 0, d.no_tile = sw[2] != 0, d.reg_prefix = sw[3] != 0, d.no_runs = sw[4] != 0,
        d.runs_always = sw[5] != 0, d.readlane = sw[6] != 0;
        const AnalogPlan pl = analog_plan(c, d);
        if (pl.error != SD_OK) {
            printf("error %d %s\nend\n", pl.error, pl.message);
            continue;
        }
        printf("plan sorted=%d K=%d tiled=%d np_runs=%d tagged=%d Ks=%d path=%d kind=%d nb=%d nthr=%d per=%d qsplit=%d reg_direct=%d npass=%d "
               "runs_q=%d skip_prob=%d need_pq=%d need_rx=%d lds=%zu chunk=%lld it_bytes=%d topk=%d nclass=%d Kq=%d prune_at=%d use_mfma=%d "
               "ablate=%d chunk_qsplit=%d\n",
               pl.sorted, pl.K, pl.tiled, pl.np_runs, pl.tagged, pl.Ks, (int)pl.path, pl.kind, pl.nb, pl.nthr, pl.per, pl.qsplit, pl.reg_direct,
               pl.npass, pl.runs_q, pl.skip_prob, pl.need_pq, pl.need_rx, pl.lds, (long long)pl.chunk, pl.it_bytes, pl.topk, pl.nclass, pl.Kq,
               pl.prune_at, pl.use_mfma, pl.ablate,
               c.op == AnalogOp::Fit ? 0 : analog_launches::qsplit(pl, (int)analog_launches::per_cell(pl, cc).gx, cc, c.Tq));
        namespace al = analog_launches;
        if (pl.tiled) put("tile_sort", al::tile_sort(pl.K, c.T, c.C));
        if (c.op == AnalogOp::Fit) {
            const int K = pl.sorted ? pl.K : pl.Ks;
            put("transpose", al::transpose(c.C, c.T));
            if (K != 0) put("sort2_tagged", al::sort2(K, c.T, c.C, pl.np_runs, c.cu_count, pl.tagged, false));
            if (K != 0) put("sort2_exact", al::sort2(K, c.T, c.C, pl.np_runs, c.cu_count, pl.tagged, true));
            put("gather_sorted", al::gather_sorted(c.C, c.cu_count));
        } else {
            put("prefix_sums", al::prefix_sums(c.T, c.C, c.cu_count, c.lds_max));
            put("rx", al::rx(c.T, c.C, c.cu_count));
            put("stage_in", al::stage_in(pl, c.Tq, cc));
            put("per_cell", al::per_cell(pl, cc));
            put("stage_out", al::stage_out(pl, c.Tq, cc));
            put("bf2", al::bf2(pl, c.C, c.Tq));
            put("transpose", al::transpose(cc, c.Tq));
            if (pl.Kq != 0) put("sort2_tagged", al::sort2(pl.Kq, c.Tq, cc, 0, c.cu_count, pl.tagged, false));
            if (pl.Kq != 0) put("sort2_exact", al::sort2(pl.Kq, c.Tq, cc, 0, c.cu_count, pl.tagged, true));
            put("slab_aux", al::slab_aux(cc, c.cu_count));
            put("slab_topk", al::slab_topk(pl, cc, c.Tq));
            put("slab_heap", al::slab_heap(c.k, c.F, cc, c.Tq, 0));
            put("status_public", al::status_public(c.C));
        }
        printf("end\n");
    }
    return 0;
}
