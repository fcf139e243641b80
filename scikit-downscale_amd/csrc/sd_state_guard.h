// Build-or-destroy guard of the fitted states (no HIP header: tests/state_guard_check.cpp compiles it with g++ alone).
#pragma once
#include "../../include/sd_downscale.h"

// Runs `body` on a freshly created state.  SD_OK: *out = st.  Anything else: the family's destroy gets st, *out stays NULL and the
// body's code is returned.
template <class State, class Destroy, class Body>
int sd_state_build(State* st, Destroy destroy, State** out, Body body) {
    *out = nullptr;
    const int rc = body();
    if (rc != SD_OK) {
        destroy(st);
        return rc;
    }
    *out = st;
    return SD_OK;
}
