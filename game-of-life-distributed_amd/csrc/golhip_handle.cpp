// golhip_handle.cpp — handle lifetime and the calls that read or write a
// board without stepping it.
#include "golhip_impl.h"
#include <cstdarg>
#include <cstdio>
#include <string>

namespace gh GOLHIP_HIDDEN {

static thread_local std::string g_err;

// Page-locked, device-mapped host buffers from golhip_host_alloc: the flip
// stream writes its entries into them straight from the kernel.
struct HostBuf {
    uintptr_t base;
    size_t bytes;
    void *dev;  // device address of base
    int device; // the device it was mapped on
};
static std::mutex g_host_mu;
static std::vector<HostBuf> g_host_bufs;

// Device address of [p, p + bytes) if it lies inside one golhip_host_alloc buffer.
void *mapped_device_ptr(const void *p, size_t bytes, int *device) {
    std::lock_guard<std::mutex> g(g_host_mu);
    const uintptr_t a = (uintptr_t)p;
    for (const HostBuf &b : g_host_bufs)
        if (a >= b.base && a + bytes <= b.base + b.bytes) {
            if (device) *device = b.device;
            return (char *)b.dev + (a - b.base);
        }
    return nullptr;
}

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int check(golhip_t h) {
    if (!h) return fail(GOLHIP_EINVAL, "null handle");
    return GOLHIP_OK;
}

int set_dev(golhip_t h) {
    HIP_OR_FAIL(hipSetDevice(h->device));
    return GOLHIP_OK;
}

// Rows per launch chunk for byte staging (<= kStageBytes of bytes; one buffer
// reused chunk after chunk).  Boards past one chunk, with a one-row last
// chunk: tests/test_gpu_io_edges.py::test_chunked_byte_io.
static constexpr int64_t kStageBytes = 64ll << 20;
static int64_t stage_rows(golhip_t h) {
    const int64_t per = std::max<int64_t>(1, kStageBytes / std::max(1, h->W));
    return std::min<int64_t>(per, h->rows);
}

// The wpl = 2 step kernels run on the interleaved pair layout; every other
// kernel reads canonical words (or is layout-agnostic: popcount, row halos).
// Converts the current board in place when the wanted layout changes.
int set_layout(golhip_t h, int il) {
    if (h->il == il) return GOLHIP_OK;
    if (h->loaded) HIP_OR_FAIL(golk::launch_convert_layout(h->cur_rows(), h->local_words(), h->il, il, h->stream));
    h->il = il;
    return GOLHIP_OK;
}

// After canonical words were written into the current buffer.
int loaded_canonical(golhip_t h) {
    h->il = 0;
    h->loaded = true;
    // a new board: the last batch's list sizes say nothing about its flip lists
    h->ft_est = 0;
    h->group_ft_est = 0;
    return set_layout(h, want_il(h));
}

static hipEvent_t take_event(golhip_t h) {
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    return e;
}

int span_begin(golhip_t h, hipStream_t st) {
    h->span_e0 = h->span_e1 = nullptr;
    if (!(h->flags & GOLHIP_FLAG_TIMING)) return GOLHIP_OK;
    h->span_e0 = take_event(h);
    h->span_e1 = take_event(h);
    h->span_stream = st;
    if (!h->span_e0 || !h->span_e1) return fail(GOLHIP_EHIP, "hipEventCreate failed");
    HIP_OR_FAIL(hipEventRecord(h->span_e0, st));
    return GOLHIP_OK;
}

int span_end(golhip_t h, int kind, bool drain) {
    if (!h->span_e1) return GOLHIP_OK;
    HIP_OR_FAIL(hipEventRecord(h->span_e1, h->span_stream));
    h->ev_pending.push_back({h->span_e0, h->span_e1, kind});
    h->span_e0 = h->span_e1 = nullptr;
    if (drain && h->ev_pending.size() >= 4096) return drain_events(h);
    return GOLHIP_OK;
}

int drain_events(golhip_t h) {
    for (auto &p : h->ev_pending) {
        HIP_OR_FAIL(hipEventSynchronize(p.e1));
        float ms = 0;
        HIP_OR_FAIL(hipEventElapsedTime(&ms, p.e0, p.e1));
        double &sum = p.kind == 1 ? h->ms.persist : p.kind == 2 ? h->ms.flip : p.kind == 3 ? h->ms.halo
                      : p.kind == 4 ? h->ms.view : h->ms.step;
        sum += ms;
        h->ev_pool.push_back(p.e0);
        h->ev_pool.push_back(p.e1);
    }
    h->ev_pending.clear();
    return GOLHIP_OK;
}

// After any stream sync: a persistent launch that timed out leaves the board
// undefined, so it is reported (loudly) and the persistent path is disabled.
static int check_persist(golhip_t h) {
    if (!h->persist_pending) return GOLHIP_OK;
    h->persist_pending = false;
    if (*h->h_err) {
        *h->h_err = 0;
        h->persistent = 0;
        return fail(GOLHIP_EHIP, "persistent step kernel timed out waiting for a neighbour workgroup "
                                 "(not all workgroups resident?); board state is undefined, persistent mode disabled");
    }
    return GOLHIP_OK;
}

// After the stream has synchronised: the K1w spin-bound flag of the launches
// it ran (reported by the call that ran them, then cleared).
int take_skew_err(golhip_t h) {
    bool err = h->skew_err && *h->skew_err;
    if (err) *h->skew_err = 0;
    if (golhip *w = h->wide; w && w->skew_err && *w->skew_err) {  // the padded torus' launches (golhip_pad.cpp)
        *w->skew_err = 0;
        err = true;
    }
    if (err) {
        return fail(GOLHIP_EHIP, "skewed-band step kernel: a band waited past its spin bound for the band below "
                                 "(board state is undefined)");
    }
    return GOLHIP_OK;
}

int sync_stream(golhip_t h) {
    HIP_OR_FAIL(hipStreamSynchronize(h->stream));
    if (int rc = take_skew_err(h)) return rc;
    return check_persist(h);
}

static int create_common(int32_t width, int32_t height, int32_t row0, int32_t rows, int32_t device, uint32_t flags,
                         bool strip, golhip_t *out) {
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    *out = nullptr;
    if (width <= 0 || height <= 0) return fail(GOLHIP_EINVAL, "bad board %dx%d", width, height);
    if (rows <= 0 || row0 < 0 || (int64_t)row0 + rows > height)
        return fail(GOLHIP_EINVAL, "bad strip rows [%d, %d) of %d", row0, row0 + rows, height);
    int ndev = 0;
    HIP_OR_FAIL(hipGetDeviceCount(&ndev));
    if (device < 0 || device >= ndev) return fail(GOLHIP_EINVAL, "device %d of %d", device, ndev);
    HIP_OR_FAIL(hipSetDevice(device));
    golhip *h = new golhip();
    h->W = width;
    h->H = height;
    h->Ww = (width + 31) / 32;
    h->row0 = row0;
    h->rows = rows;
    h->strip = strip;
    h->device = device;
    h->flags = flags;
    h->phys_rows = (int64_t)rows + 2 * kHalo;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, device) == hipSuccess) h->cu_count = prop.multiProcessorCount;
        if (h->cu_count <= 0) h->cu_count = 256;
        h->dev_cu = h->cu_count;
    }
    const size_t bytes = (size_t)h->phys_rows * h->Ww * sizeof(uint32_t);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e == hipSuccess) h->own_stream = true;
    if (e == hipSuccess) e = hipMalloc(&h->buf[0], bytes);
    if (e == hipSuccess) e = hipMalloc(&h->buf[1], bytes);
    // zeroed on the handle's own stream: it is non-blocking, so a plain
    // hipMemset (null stream, asynchronous for device memory) could still be
    // running when the first load / fill_random on `stream` writes the board
    if (e == hipSuccess) e = hipMemsetAsync(h->buf[0], 0, bytes, h->stream);
    if (e == hipSuccess) e = hipMemsetAsync(h->buf[1], 0, bytes, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = hipMalloc(&h->d_scalars, 4 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipHostMalloc(&h->h_scalars, 4 * sizeof(unsigned long long), hipHostMallocDefault);
    if (e != hipSuccess) {
        int code = (e == hipErrorOutOfMemory) ? GOLHIP_ENOMEM : GOLHIP_EHIP;
        fail(code, "allocating %zu bytes x2: %s", bytes, hipGetErrorString(e));
        golhip_destroy(h);
        return code;
    }
    *out = h;
    return GOLHIP_OK;
}

// Alive count of this handle's rows at the current turn (h->mu held): the
// fused count of the last launch if it belongs to this turn, else a popcount.
static int alive_count_locked(golhip_t h, uint64_t *count, int64_t *at_turn) {
    if (int rc = set_dev(h)) return rc;
    if (h->alive_turn != h->turns) {
        HIP_OR_FAIL(hipMemsetAsync(h->d_scalars, 0, sizeof(unsigned long long), h->stream));
        HIP_OR_FAIL(golk::launch_popcount(h->cur_rows(), h->local_words(), h->d_scalars, h->stream));
        h->alive_turn = h->turns;
    }
    HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars, h->d_scalars, sizeof(unsigned long long), hipMemcpyDeviceToHost, h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    *count = h->h_scalars[0];
    if (at_turn) *at_turn = h->alive_turn;
    return GOLHIP_OK;
}

}  // namespace gh

using namespace gh;

extern "C" {

const char *golhip_version(void) { return "golhip 0.1 (gfx950)"; }

const char *golhip_last_error(void) { return g_err.c_str(); }

int golhip_device_count(int32_t *n) {
    if (!n) return fail(GOLHIP_EINVAL, "n is null");
    int c = 0;
    HIP_OR_FAIL(hipGetDeviceCount(&c));
    *n = c;
    return GOLHIP_OK;
}

int golhip_host_alloc(uint64_t bytes, void **out) {
    if (!out || bytes == 0) return fail(GOLHIP_EINVAL, "bad host allocation");
    *out = nullptr;
    void *p = nullptr, *d = nullptr;
    hipError_t e = hipHostMalloc(&p, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(GOLHIP_ENOMEM, "hipHostMalloc(%llu): %s", (unsigned long long)bytes, hipGetErrorString(e));
    e = hipHostGetDevicePointer(&d, p, 0);
    if (e != hipSuccess) {
        (void)hipHostFree(p);
        return fail(GOLHIP_EHIP, "hipHostGetDevicePointer: %s", hipGetErrorString(e));
    }
    int device = 0;
    (void)hipGetDevice(&device);
    std::lock_guard<std::mutex> g(g_host_mu);
    g_host_bufs.push_back({(uintptr_t)p, (size_t)bytes, d, device});
    *out = p;
    return GOLHIP_OK;
}

int golhip_host_free(void *p) {
    if (!p) return GOLHIP_OK;
    {
        std::lock_guard<std::mutex> g(g_host_mu);
        auto it = std::find_if(g_host_bufs.begin(), g_host_bufs.end(),
                               [&](const HostBuf &b) { return b.base == (uintptr_t)p; });
        if (it == g_host_bufs.end()) return fail(GOLHIP_EINVAL, "not a golhip_host_alloc buffer");
        g_host_bufs.erase(it);
    }
    HIP_OR_FAIL(hipHostFree(p));
    return GOLHIP_OK;
}

int golhip_host_link_probe(int32_t device, uint64_t bytes, int32_t reps, double *kernel_write_gbps,
                           double *dma_d2h_gbps) {
    if (!kernel_write_gbps || !dma_d2h_gbps || bytes < 4096 || bytes % 16 || reps < 1 || reps > 1000)
        return fail(GOLHIP_EINVAL, "host link probe: bytes >= 4096, a multiple of 16; 1 <= reps <= 1000");
    *kernel_write_gbps = *dma_d2h_gbps = 0;
    HIP_OR_FAIL(hipSetDevice(device));
    int cus = 0;
    HIP_OR_FAIL(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
    // the buffer K5 writes into: golhip_host_alloc's kind (hipHostMalloc, device-mapped)
    void *host = nullptr, *host_dev = nullptr, *dev = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    hipError_t e = hipHostMalloc(&host, (size_t)bytes, hipHostMallocDefault);
    if (e == hipSuccess) e = hipHostGetDevicePointer(&host_dev, host, 0);
    if (e == hipSuccess) e = hipMalloc(&dev, (size_t)bytes);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&st, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipMemsetAsync(dev, 0x5a, (size_t)bytes, st);
    // K5's own shape: 256-thread blocks, a few per CU, 16-byte stores
    const int blocks = 4 * cus;
    float kms = 0, dms = 0;
    if (e == hipSuccess) e = golk::launch_host_write_probe(host_dev, bytes, blocks, 0, st);  // warm (page mapping)
    if (e == hipSuccess) e = hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int r = 0; e == hipSuccess && r < reps; ++r) e = golk::launch_host_write_probe(host_dev, bytes, blocks, r + 1, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&kms, e0, e1);
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int r = 0; e == hipSuccess && r < reps; ++r)
        e = hipMemcpyAsync(host, dev, (size_t)bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&dms, e0, e1);
    // the last kernel pass's pattern must be in host memory (tag reps: word 0 == reps)
    if (e == hipSuccess && reps >= 1) {
        // (the DMA passes overwrote it with 0x5a bytes: check those instead)
        const uint32_t w = static_cast<const uint32_t *>(host)[bytes / 4 - 1];
        if (w != 0x5a5a5a5au) e = hipErrorUnknown;
    }
    if (e1) (void)hipEventDestroy(e1);
    if (e0) (void)hipEventDestroy(e0);
    if (st) (void)hipStreamDestroy(st);
    if (dev) (void)hipFree(dev);
    if (host) (void)hipHostFree(host);
    if (e != hipSuccess) return fail(GOLHIP_EHIP, "host link probe: %s", hipGetErrorString(e));
    *kernel_write_gbps = kms > 0 ? (double)bytes * reps / (kms * 1e-3) / 1e9 : 0;
    *dma_d2h_gbps = dms > 0 ? (double)bytes * reps / (dms * 1e-3) / 1e9 : 0;
    return GOLHIP_OK;
}

int golhip_create(int32_t width, int32_t height, int32_t device, uint32_t flags, golhip_t *out) {
    return create_common(width, height, 0, height, device, flags, false, out);
}

int golhip_create_strip(int32_t width, int32_t height, int32_t row0, int32_t rows, int32_t device, uint32_t flags,
                        golhip_t *out) {
    return create_common(width, height, row0, rows, device, flags, true, out);
}

int golhip_destroy(golhip_t h) {
    if (!h) return GOLHIP_OK;
    int rc = GOLHIP_OK;
    HIP_RC(hipSetDevice(h->device));
    if (h->stream) HIP_RC(hipStreamSynchronize(h->stream));
    if (int prc = pad_destroy(h); prc && rc == GOLHIP_OK) rc = prc;
    for (auto &p : h->ev_pending) {
        HIP_RC(hipEventDestroy(p.e0));
        HIP_RC(hipEventDestroy(p.e1));
    }
    for (auto e : h->ev_pool) HIP_RC(hipEventDestroy(e));
    if (h->comm && ncclCommDestroy(h->comm) != ncclSuccess && rc == GOLHIP_OK)
        rc = fail(GOLHIP_ERCCL, "ncclCommDestroy failed");
    HIP_RC(hipFree(h->buf[0]));
    HIP_RC(hipFree(h->buf[1]));
    HIP_RC(hipFree(h->d_scalars));
    if (h->h_scalars) HIP_RC(hipHostFree(h->h_scalars));
    HIP_RC(hipFree(h->d_blk.p));
    HIP_RC(hipFree(h->d_xy.p));
    HIP_RC(hipFree(h->d_run.p));
    HIP_RC(hipFree(h->d_ftstatus.p));
    HIP_RC(hipFree(h->d_ftticket.p));
    HIP_RC(hipFree(h->d_ftctl.p));
    HIP_RC(hipFree(h->d_ftdone.p));
    HIP_RC(hipFree(h->d_ev.p));
    HIP_RC(hipFree(h->d_goff.p));
    if (h->g_stage) HIP_RC(hipHostFree(h->g_stage));
    HIP_RC(hipFree(h->d_stage.p));
    HIP_RC(hipFree(h->d_vcount.p));
    HIP_RC(hipFree(h->d_sync));
    HIP_RC(hipFree(h->d_trace));
    HIP_RC(hipFree(h->backup.p));
    HIP_RC(hipFree(h->lds_edge.p));
    if (h->h_err) HIP_RC(hipHostFree(h->h_err));
    if (h->skew_err) HIP_RC(hipHostFree(h->skew_err));
    if (h->xport_host) HIP_RC(hipHostFree(h->xport_host));
    if (h->own_stream && h->stream) HIP_RC(hipStreamDestroy(h->stream));
    delete h;
    return rc;
}

int golhip_set_stream(golhip_t h, void *s) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    if (h->own_stream) HIP_OR_FAIL(hipStreamDestroy(h->stream));
    h->own_stream = false;
    h->stream = (hipStream_t)s;
    if (h->wide) h->wide->stream = h->stream;
    return GOLHIP_OK;
}

void *golhip_stream(golhip_t h) { return h ? (void *)h->stream : nullptr; }

int golhip_load_bytes(golhip_t h, const uint8_t *cells) {
    if (int rc = check(h)) return rc;
    if (!cells) return fail(GOLHIP_EINVAL, "cells is null");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    const int64_t chunk = stage_rows(h);
    if (int rc = h->d_stage.ensure(h, chunk * h->W)) return rc;
    for (int64_t r = 0; r < h->rows; r += chunk) {
        const int64_t n = std::min<int64_t>(chunk, h->rows - r);
        HIP_OR_FAIL(hipMemcpyAsync(h->d_stage.p, cells + r * h->W, (size_t)(n * h->W), hipMemcpyHostToDevice, h->stream));
        HIP_OR_FAIL(golk::launch_pack(h->d_stage.p, h->cur_rows() + r * h->Ww, h->W, h->Ww, (int)n, h->stream));
    }
    if (int rc = loaded_canonical(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    h->turns = 0;
    h->alive_turn = -1;
    h->flips_valid = false;
    return GOLHIP_OK;
}

int golhip_load_bits(golhip_t h, const uint32_t *words) {
    if (int rc = check(h)) return rc;
    if (!words) return fail(GOLHIP_EINVAL, "words is null");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    HIP_OR_FAIL(hipMemcpyAsync(h->cur_rows(), words, (size_t)h->local_words() * 4, hipMemcpyHostToDevice, h->stream));
    // the caller's bits of columns >= width are no cells (golhip.h): popcount, hash and K3 run over whole words
    HIP_OR_FAIL(golk::launch_clear_row_tail(h->cur_rows(), h->W, h->Ww, h->rows, h->stream));
    if (int rc = loaded_canonical(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    h->turns = 0;
    h->alive_turn = -1;
    h->flips_valid = false;
    return GOLHIP_OK;
}

int golhip_fill_random(golhip_t h, uint64_t seed) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    HIP_OR_FAIL(golk::launch_fill_random(h->cur_rows(), h->W, h->Ww, h->rows, h->row0, seed, h->stream));
    if (int rc = loaded_canonical(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    h->turns = 0;
    h->alive_turn = -1;
    h->flips_valid = false;
    return GOLHIP_OK;
}

int golhip_sync(golhip_t h) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (int rc_ = sync_stream(h)) return rc_;
    return GOLHIP_OK;
}

int golhip_turn(golhip_t h, int64_t *t) {
    if (int rc = check(h)) return rc;
    if (!t) return fail(GOLHIP_EINVAL, "null out");
    *t = h->turns.load();
    return GOLHIP_OK;
}

int golhip_alive_count(golhip_t h, uint64_t *count, int64_t *at_turn) {
    if (int rc = check(h)) return rc;
    if (!count) return fail(GOLHIP_EINVAL, "null out");
    std::lock_guard<std::mutex> g(h->mu);
    return alive_count_locked(h, count, at_turn);
}

int golhip_alive_count_global(golhip_t h, uint64_t *count, int64_t *at_turn) {
    if (int rc = check(h)) return rc;
    if (!count) return fail(GOLHIP_EINVAL, "null out");
    // one critical section: local count, copy and allreduce all belong to the
    // same turn (a concurrent golhip_step cannot advance the board between them)
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = alive_count_locked(h, count, at_turn)) return rc;
    if (!h->ringed()) return GOLHIP_OK;
    if (!h->comm) {
        // test transport: the sum rides the same host callback (prev = next =
        // -1 marks an allreduce of one uint64, golhip_test_transport_fn)
        unsigned long long in = *count, out = 0;
        if (int r = h->xport(h->xport_user, -1, -1, &in, nullptr, &out, nullptr, (int64_t)sizeof in))
            return fail(GOLHIP_ERCCL, "test transport allreduce returned %d", r);
        *count = out;
        return GOLHIP_OK;
    }
    // the ring's RCCL communicator (also a one-rank ring: the same call as at 8 GPUs)
    HIP_OR_FAIL(hipMemcpyAsync(h->d_scalars + 3, h->d_scalars, sizeof(unsigned long long), hipMemcpyDeviceToDevice,
                               h->stream));
    NCCL_OR_FAIL(ncclAllReduce(h->d_scalars + 3, h->d_scalars + 3, 1, ncclUint64, ncclSum, h->comm, h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars + 3, h->d_scalars + 3, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    *count = h->h_scalars[3];
    return GOLHIP_OK;
}

int golhip_snapshot_bytes(golhip_t h, uint8_t *out) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    const int64_t chunk = stage_rows(h);
    if (int rc = h->d_stage.ensure(h, chunk * h->W)) return rc;
    for (int64_t r = 0; r < h->rows; r += chunk) {
        const int64_t n = std::min<int64_t>(chunk, h->rows - r);
        HIP_OR_FAIL(golk::launch_unpack(h->cur_rows() + r * h->Ww, h->d_stage.p, h->W, h->Ww, (int)n, h->il, h->stream));
        HIP_OR_FAIL(hipMemcpyAsync(out + r * h->W, h->d_stage.p, (size_t)(n * h->W), hipMemcpyDeviceToHost, h->stream));
    }
    if (int rc_ = sync_stream(h)) return rc_;
    return GOLHIP_OK;
}

int golhip_snapshot_bits(golhip_t h, uint32_t *out) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    const int il = h->il;
    HIP_OR_FAIL(golk::launch_convert_layout(h->cur_rows(), h->local_words(), il, 0, h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(out, h->cur_rows(), (size_t)h->local_words() * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_OR_FAIL(golk::launch_convert_layout(h->cur_rows(), h->local_words(), 0, il, h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    return GOLHIP_OK;
}

int golhip_snapshot_rows(golhip_t h, int32_t row, int32_t nrows, uint32_t *out) {
    if (int rc = check(h)) return rc;
    if (!out || row < 0 || nrows < 0 || (int64_t)row + nrows > h->rows)
        return fail(GOLHIP_EINVAL, "rows [%d, %d) not in [0, %d)", row, row + nrows, h->rows);
    if (nrows == 0) return GOLHIP_OK;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    // a row holds whole pairs / quads in their layouts, so the range converts alone
    // (a pair-layout row may start 8 bytes off a 16-byte boundary: launch_convert_layout goes by pairs then)
    uint32_t *p = h->cur_rows() + (int64_t)row * h->Ww;
    const int64_t n = (int64_t)nrows * h->Ww;
    HIP_OR_FAIL(golk::launch_convert_layout(p, n, h->il, 0, h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(out, p, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
    HIP_OR_FAIL(golk::launch_convert_layout(p, n, 0, h->il, h->stream));
    return sync_stream(h);
}

int golhip_board_hash(golhip_t h, uint64_t *hash) {
    if (int rc = check(h)) return rc;
    if (!hash) return fail(GOLHIP_EINVAL, "null out");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    HIP_OR_FAIL(hipMemsetAsync(h->d_scalars + 2, 0, sizeof(unsigned long long), h->stream));
    HIP_OR_FAIL(golk::launch_hash(h->cur_rows(), h->local_words(), (int64_t)h->row0 * h->Ww, h->d_scalars + 2, h->il,
                                  h->stream));
    HIP_OR_FAIL(hipMemcpyAsync(h->h_scalars + 2, h->d_scalars + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost,
                               h->stream));
    if (int rc_ = sync_stream(h)) return rc_;
    *hash = h->h_scalars[2];
    return GOLHIP_OK;
}

int golhip_perf(golhip_t h, golhip_perf_t *out) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(GOLHIP_EINVAL, "null out");
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (int rc = sync_stream(h)) return rc;
    if (int rc = drain_events(h)) return rc;
    if (h->wide) {  // the padded torus' timed launches are this handle's step launches
        if (int rc = drain_events(h->wide)) return rc;
        h->ms.step += h->wide->ms.step;
        h->wide->ms = Millis{};
    }
    memset(out, 0, sizeof *out);
    const Counters &n = h->n;
    out->turns = h->turns;
    out->step_launches = n.step_launches;
    out->step_turns = n.step_turns;
    out->step_kernel_ms = h->ms.step;
    out->persist_launches = n.persist_launches;
    out->persist_turns = n.persist_turns;
    out->persist_kernel_ms = h->ms.persist;
    out->persist_fallbacks = h->persist_fallbacks;
    out->flip_launches = n.flip_launches;
    out->flip_kernel_ms = h->ms.flip;
    out->flip_entries = n.flip_entries;
    out->flip_fallbacks = h->flip_fallbacks;
    out->cell_updates = (int64_t)h->W * h->rows * (n.step_turns + n.persist_turns + n.flip_launches);
    out->alg_bytes = out->cell_updates / 4;
    out->halo_bytes = n.halo_bytes;
    const bool halo = h->halo_mode();
    out->tb_depth = depth_cap(h, halo);
    out->rows_per_wave = rows_per_wave_for(h, next_depth(h, h->tb_depth, halo));
    out->kernel_variant = h->last_variant;
    out->skew_launches = n.skew_launches;
    out->halo_exchanges = n.halo_exchanges;
    out->halo_ms = h->ms.halo;
    out->skew_half_launches = n.skew_half_launches;
    out->lds_launches = n.lds_launches;
    out->pair_launches = n.pair_launches;
    out->pair_turns = n.pair_turns;
    out->flip_resident_launches = n.flip_resident;
    out->view_frames = n.view_frames;
    out->view_kernel_ms = h->ms.view;
    out->pad_launches = n.pad_launches;
    out->rule_launches = n.rule_launches;
    out->words_per_lane = (h->W % 32 == 0 || h->plane) ? wpl_for(h) : 0;  // (a plane: K15's one word a lane at any width)
    out->persist_depth = h->W % 32 == 0 ? persist_depth_for(h, wpl_for(h)) : 0;
    return GOLHIP_OK;
}

int golhip_persist_trace_waves(golhip_t h, uint64_t *out, int64_t n) {
    if (int rc = check(h)) return rc;
    if (!out || n < 0 || n > kTraceWords - 8) return fail(GOLHIP_EINVAL, "bad out");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->d_trace) return fail(GOLHIP_EINVAL, "set option \"trace\" first");
    if (int rc = set_dev(h)) return rc;
    if (int rc = sync_stream(h)) return rc;
    HIP_OR_FAIL(hipMemcpy(out, h->d_trace + 8, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return GOLHIP_OK;
}

int golhip_persist_trace(golhip_t h, uint64_t out[5]) {
    if (int rc = check(h)) return rc;
    if (!out) return fail(GOLHIP_EINVAL, "null out");
    std::lock_guard<std::mutex> g(h->mu);
    if (!h->d_trace) return fail(GOLHIP_EINVAL, "set option \"trace\" first");
    if (int rc = set_dev(h)) return rc;
    if (int rc = sync_stream(h)) return rc;
    HIP_OR_FAIL(hipMemcpy(out, h->d_trace, 5 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    HIP_OR_FAIL(hipMemsetAsync(h->d_trace, 0, 8 * sizeof(unsigned long long), h->stream));
    HIP_OR_FAIL(hipStreamSynchronize(h->stream));
    return GOLHIP_OK;
}

int golhip_perf_reset(golhip_t h) {
    if (int rc = check(h)) return rc;
    std::lock_guard<std::mutex> g(h->mu);
    if (int rc = set_dev(h)) return rc;
    if (int rc = drain_events(h)) return rc;
    if (h->wide) {
        if (int rc = drain_events(h->wide)) return rc;
        h->wide->ms = Millis{};
    }
    // (turns, persist_fallbacks, flip_fallbacks and the plan caches stay)
    h->n = Counters{};
    h->ms = Millis{};
    return GOLHIP_OK;
}

}  // extern "C"
