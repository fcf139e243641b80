// Host driver of the ARRM launch plan (scikit-downscale_amd/csrc/sd_arrm_plan.h) for tests/test_arrm_plan.py.
//   in:  "T C ld max_breakpoints lds_max cu_count" per line
//   out: "error <code> <message>", or "plan half B start width nacc slices", "select gx block lds", "accum gx gy block lds",
//        "predict gx gy block lds" (arrm_predict_launch of Tq = T rows), "upper <mid of every final window, ascending left>", "lower <final flag of left = 0 .. start + 4>"; then "end".
#include <iostream>

#include "sd_arrm_plan.h"

int main() {
    ArrmCall c;
    long long lds;
    while (std::cin >> c.T >> c.C >> c.ld >> c.max_breakpoints >> lds >> c.cu_count) {
        c.lds_max = (size_t)lds;
        const ArrmPlan p = arrm_plan(c);
        if (p.error != SD_OK) {
            std::cout << "error " << p.error << " " << p.message << "\nend\n";
            continue;
        }
        std::cout << "plan " << p.half << " " << p.B << " " << p.start << " " << p.width << " " << p.nacc << " " << p.slices << "\n";
        std::cout << "select " << p.select.gx << " " << p.select.block << " " << p.select.lds << "\n";
        std::cout << "accum " << p.accum.gx << " " << p.accum.gy << " " << p.accum.block << " " << p.accum.lds << "\n";
        const ArrmLaunch q = arrm_predict_launch(c.T, c.C, p.B);  // (a query of as many rows as the fit has samples)
        std::cout << "predict " << q.gx << " " << q.gy << " " << q.block << " " << q.lds << "\n";
        std::cout << "upper";
        for (int64_t left = p.start - p.width; left + p.width <= c.T; ++left)
            if (sdarrm::upper_final(left, p.width, c.T)) std::cout << " " << sdarrm::mid_of(left, left + p.width);
        std::cout << "\nlower";
        for (int64_t left = 0; left <= p.start + 4; ++left) std::cout << " " << (sdarrm::lower_final(left, p.width) ? 1 : 0);
        std::cout << "\nend\n";
    }
    return 0;
}
