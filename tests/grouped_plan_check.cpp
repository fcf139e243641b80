// Host driver of the grouped-regression plan (scikit-downscale_amd/csrc/sd_grouped_plan.h) for tests/test_grouped_host.py.
//   in:  "tile F n window lds_max"   out: "tile cells run slots lds"
//   in:  "keys T n" then T keys      out: "error <code> <first_bad>" or "order <T indices>", "off <n+1 offsets>", "fitted w <n flags>"
//                                         for w = 0 and 1
#include <iostream>

#include "sd_grouped_plan.h"

int main() {
    std::string cmd;
    while (std::cin >> cmd) {
        if (cmd == "tile") {
            int F, n, w;
            size_t lds;
            std::cin >> F >> n >> w >> lds;
            const GroupedWindowTile t = grouped_window_tile(F, n, w, lds);
            std::cout << "tile " << t.cells << " " << t.run << " " << t.slots << " " << t.lds << "\n";
        } else {
            int64_t T;
            int n;
            std::cin >> T >> n;
            std::vector<int32_t> key(T);
            for (auto& k : key) std::cin >> k;
            const GroupedKeyTable p = grouped_key_table(key.data(), T, n);
            if (p.err != SD_OK) {
                std::cout << "error " << p.err << " " << p.first_bad << "\n";
                continue;
            }
            std::cout << "order";
            for (int32_t t : p.order) std::cout << " " << t;
            std::cout << "\noff";
            for (int64_t o : p.off) std::cout << " " << o;
            std::cout << "\n";
            for (int w = 0; w < 2 && w < n; ++w) {
                std::cout << "fitted " << w;
                for (int32_t f : grouped_fitted(p.cnt, w)) std::cout << " " << f;
                std::cout << "\n";
            }
        }
    }
    return 0;
}
