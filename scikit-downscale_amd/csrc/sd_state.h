// Host scaffolding shared by every family with a fitted state (sd_bcsd.hip, sd_analog.hip, sd_linreg.hip, sd_zscore.hip,
// sd_grouped.hip, sd_arrm.hip, sd_qm.hip): the buffer list of a state and what walks it, the per-cell status in both directions,
// small uploads, and the host-buffer form of an entry point (that one also in sd_regrid.hip and sd_resample.hip, which have no
// state).  Host code only; a family keeps its struct, its buffer list, its plan, its kernels and the argument checks of its entry
// points.  BCSD and the analogs fold the status of a predict call on the device (status_public_kernel: the fit's code before the
// call's; analog_status_public_kernel); of the two, only BCSD's export and status query go through sd_status_fold.
#pragma once
#include <algorithm>
#include <initializer_list>
#include <vector>

#include "sd_internal.h"
#include "sd_state_guard.h"

// ---- the device buffers of a state, named once per state ------------------------------------------------------------------------
struct sd_buf {
    void** slot;   // the state's pointer
    size_t bytes;
    bool zero;     // cleared on allocation
};
template <typename T>
sd_buf sd_buf_of(T* const& field, size_t count, bool zero = false) {
    return {(void**)&field, sizeof(T) * count, zero};
}

inline int sd_state_alloc(sd_ctx* ctx, const std::vector<sd_buf>& bufs) {
    for (const sd_buf& b : bufs) {
        SD_HIP(sd_pool_malloc(ctx, b.slot, b.bytes));
        if (b.zero) SD_HIP(hipMemsetAsync(*b.slot, 0, b.bytes, ctx->stream));
    }
    return SD_OK;
}

// set device, drain the stream, release what was allocated, delete
template <class State, class Bufs>
int sd_state_destroy(State* st, Bufs bufs_of) {
    if (!st) return SD_OK;
    if (st->ctx) {
        (void)hipSetDevice(st->ctx->device);
        (void)hipStreamSynchronize(st->ctx->stream);
    }
    for (const sd_buf& b : bufs_of(st))
        if (*b.slot) sd_pool_release(st->ctx, *b.slot);
    delete st;
    return SD_OK;
}

// export (device to host) / import (host to device): one host pointer per buffer, in the order of the list; NULL skips its buffer.
// Queued on ctx->stream, not waited for.
inline int sd_state_copy(sd_ctx* ctx, const std::vector<sd_buf>& bufs, std::initializer_list<const void*> host, hipMemcpyKind kind) {
    size_t i = 0;
    for (const void* h : host) {
        if (i == bufs.size()) break;
        const sd_buf& b = bufs[i++];
        if (!h) continue;
        void* const hp = const_cast<void*>(h);
        const bool in = kind == hipMemcpyHostToDevice;
        SD_HIP(hipMemcpyAsync(in ? *b.slot : hp, in ? hp : *b.slot, b.bytes, kind, ctx->stream));
    }
    return SD_OK;
}

// ---- per-cell status ------------------------------------------------------------------------------------------------------------
// public codes of an import -> internal bits (all clear without codes)
inline std::vector<int32_t> sd_status_bits(const int32_t* cell_status, int64_t C) {
    std::vector<int32_t> bits((size_t)C, 0);
    if (cell_status)
        for (int64_t c = 0; c < C; ++c) bits[c] = sd_internal_status(cell_status[c]);
    return bits;
}

// internal bits -> public codes: what fit found (fit_bits) or'ed with what this call found (call_bits, may be NULL), both on the
// device.  Drains ctx->stream, also when no status is asked for: every export and predict ends here.
inline int sd_status_fold(sd_ctx* ctx, const int32_t* fit_bits, const int32_t* call_bits, int64_t C, int32_t* cell_status) {
    std::vector<int32_t> a, b;
    if (cell_status) {
        a.resize((size_t)C);
        b.assign((size_t)C, 0);
        SD_HIP(hipMemcpyAsync(a.data(), fit_bits, sizeof(int32_t) * C, hipMemcpyDeviceToHost, ctx->stream));
        if (call_bits) SD_HIP(hipMemcpyAsync(b.data(), call_bits, sizeof(int32_t) * C, hipMemcpyDeviceToHost, ctx->stream));
    }
    SD_HIP(hipStreamSynchronize(ctx->stream));
    for (size_t c = 0; c < a.size(); ++c) cell_status[c] = sd_public_status(a[c] | b[c]);
    return SD_OK;
}

// the status bits of one predict call: [C], cleared
inline int sd_status_scratch(sd_ctx* ctx, sd_scratch& s, int64_t C) {
    SD_HIP(s.alloc(ctx, sizeof(int32_t) * C));
    SD_HIP(hipMemsetAsync(s.p, 0, sizeof(int32_t) * C, ctx->stream));
    return SD_OK;
}

// ---- uploads --------------------------------------------------------------------------------------------------------------------
// a small host table -> scratch (queued on ctx->stream)
template <typename Tv>
int upload(sd_ctx* ctx, sd_scratch& s, const std::vector<Tv>& v) {
    SD_HIP(s.alloc(ctx, sizeof(Tv) * std::max<size_t>(v.size(), 1)));
    SD_HIP(hipMemcpyAsync(s.p, v.data(), sizeof(Tv) * v.size(), hipMemcpyHostToDevice, ctx->stream));
    return SD_OK;
}

// The host-buffer form of an entry point: every field gets device scratch, the inputs go up, `call` (the resident entry point)
// gets the device pointers in the order of the fields, the outputs come down, the stream is drained.  A field whose host pointer
// is NULL (an optional input or output) gets a NULL device pointer and no copy.
struct sd_host_field {
    void* host;
    size_t bytes;
    bool out;
};
inline sd_host_field sd_in(const void* host, size_t bytes) { return {const_cast<void*>(host), bytes, false}; }
inline sd_host_field sd_out(void* host, size_t bytes) { return {host, bytes, true}; }

template <size_t N, class Call>
int with_device_copies(sd_ctx* ctx, const sd_host_field (&f)[N], Call call) {
    SD_HIP(hipSetDevice(ctx->device));
    sd_scratch dev[N];
    void* p[N];
    for (size_t i = 0; i < N; ++i) {
        if (f[i].host) SD_HIP(dev[i].alloc(ctx, f[i].bytes));
        p[i] = dev[i].p;
    }
    for (size_t i = 0; i < N; ++i)
        if (f[i].host && !f[i].out) SD_TRY(sd_copy_h2d(ctx, p[i], f[i].host, f[i].bytes));
    SD_TRY(call((void* const*)p));
    for (size_t i = 0; i < N; ++i)
        if (f[i].host && f[i].out) SD_TRY(sd_copy_d2h(ctx, f[i].host, p[i], f[i].bytes));
    SD_HIP(hipStreamSynchronize(ctx->stream));
    return SD_OK;
}
