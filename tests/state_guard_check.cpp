// Host driver of the build-or-destroy guard (scikit-downscale_amd/csrc/sd_state_guard.h) for tests/test_state_guard.py.
//   in:  the code the body returns, one per line
//   out: "rc <returned code> destroys <calls of destroy> out <null | state>", where "state" means *out is the state that was handed in
#include <iostream>

#include "sd_state_guard.h"

struct fake_state {
    int* destroys;
};

int fake_destroy(fake_state* st) {
    ++*st->destroys;
    delete st;
    return SD_OK;
}

int main() {
    int code;
    while (std::cin >> code) {
        int destroys = 0;
        fake_state* const st = new fake_state{&destroys};
        fake_state* out = reinterpret_cast<fake_state*>(&destroys);  // (not NULL and not the state: the guard must write it)
        const int rc = sd_state_build(st, fake_destroy, &out, [&]() -> int { return code; });
        std::cout << "rc " << rc << " destroys " << destroys << " out " << (out == nullptr ? "null" : out == st ? "state" : "other") << "\n";
        if (out == st) delete st;
    }
    return 0;
}
