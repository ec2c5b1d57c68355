// golhip_ckpt.cpp — checkpoints of a board: the shadow copy
// behind the enqueued turns (K8, gol_ckpt.hip), its drain to a file behind the
// following turns, and the verified load.  The file layer is gol_ckpt_file.h.
#include "golhip_impl.h"

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>
#include <chrono>
#include <string>
#include <thread>

#include "gol_ckpt_file.h"
#include "gol_image_file.h"  // the automatic chunk rule (one definition for both jobs)

namespace gh GOLHIP_HIDDEN {

// ---- shared with golhip_image.cpp (declared in golhip_impl.h) ---------------
double ms_since(Clock::time_point t0) { return std::chrono::duration<double, std::milli>(Clock::now() - t0).count(); }

int chunk_rows_for(const golhip_ckpt_opts_t *opts, int64_t row_bytes, int *out) {
    const int32_t want = opts ? opts->chunk_rows : 0;
    if (want < 0) return fail(GOLHIP_EINVAL, "chunk_rows %d", want);
    *out = (int)golimg::chunk_rows_for(want, row_bytes, INT32_MAX);
    return GOLHIP_OK;
}

bool write_all(int fd, const void *p, size_t bytes, uint64_t off) {
    const char *c = static_cast<const char *>(p);
    while (bytes) {
        const ssize_t w = pwrite(fd, c, bytes, (off_t)off);
        if (w < 0 && errno == EINTR) continue;
        if (w <= 0) return false;
        c += w;
        off += (uint64_t)w;
        bytes -= (size_t)w;
    }
    return true;
}

bool read_all(int fd, void *p, size_t bytes, uint64_t off) {
    char *c = static_cast<char *>(p);
    while (bytes) {
        const ssize_t r = pread(fd, c, bytes, (off_t)off);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) return false;
        c += r;
        off += (uint64_t)r;
        bytes -= (size_t)r;
    }
    return true;
}

bool file_commit(int fd, const std::string &tmp, const std::string &path, const void *head, size_t head_bytes, bool ok,
                 const char **what) {
    *what = nullptr;
    int err = 0;
    auto bad = [&](const char *w) {
        if (!*what) {
            *what = w;
            err = errno;
        }
        ok = false;
    };
    if (ok && !write_all(fd, head, head_bytes, 0)) bad("write");
    if (ok && fsync(fd) != 0) bad("fsync");
    if (fd >= 0 && close(fd) != 0) bad("close");
    if (ok && rename(tmp.c_str(), path.c_str()) != 0) bad("rename");
    if (!ok && fd >= 0) unlink(tmp.c_str());
    if (*what) errno = err;
    return ok;
}

void drain_set(CkptDrain &d) {
    {
        std::lock_guard<std::mutex> g(d.mu);
        d.drained = true;
    }
    d.cv.notify_all();
}

void drain_wait_earlier(golhip_t *hs, int32_t n) {
    for (int i = 0; i < n; ++i) {
        std::shared_ptr<CkptDrain> d;
        {
            std::lock_guard<std::mutex> g(hs[i]->drain_mu);
            d = hs[i]->ckpt_drain;
        }
        if (d) {
            std::unique_lock<std::mutex> lk(d->mu);
            d->cv.wait(lk, [&] { return d->drained; });
        }
    }
}

int shadow_alloc(golhip_t *hs, int32_t n, const char *what, std::vector<ShadowPart> &parts, int *max_rows) {
    parts.resize((size_t)n);
    *max_rows = 0;
    int rc = GOLHIP_OK;
    for (int i = 0; i < n && !rc; ++i) {
        ShadowPart &p = parts[(size_t)i];
        p.device = hs[i]->device;
        p.row0 = hs[i]->row0;
        p.rows = hs[i]->rows;
        *max_rows = std::max(*max_rows, hs[i]->rows);
        HIP_RC(hipSetDevice(p.device));
        if (!rc) {
            if (hipMalloc(&p.shadow, (size_t)hs[i]->local_words() * 4) != hipSuccess)
                rc = fail(GOLHIP_ENOMEM, "%s shadow of %lld bytes", what, (long long)hs[i]->local_words() * 4);
        }
        if (!rc) HIP_RC(hipMalloc(&p.d_sums, 2 * sizeof(unsigned long long)));
        if (!rc) HIP_RC(hipEventCreate(&p.k0));
        if (!rc) HIP_RC(hipEventCreate(&p.k1));
        for (int j = 0; j < i && !p.side; ++j)
            if (parts[(size_t)j].device == p.device) p.side = parts[(size_t)j].side;
        if (!rc && !p.side) {
            HIP_RC(hipStreamCreateWithFlags(&p.side, hipStreamNonBlocking));
            p.own_side = !rc;
        }
    }
    return rc;
}

int shadow_enqueue(golhip_t *hs, int32_t n, std::vector<ShadowPart> &parts, const std::shared_ptr<CkptDrain> &drain,
                   int64_t *turn) {
    int rc = GOLHIP_OK;
    // one critical section over the group: every strip at one turn, one kernel a strip
    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    *turn = hs[0]->turns.load();
    for (int i = 1; i < n && !rc; ++i)
        if (hs[i]->turns.load() != *turn)
            rc = fail(GOLHIP_EINVAL, "strip %d is at turn %lld, strip 0 at %lld", i, (long long)hs[i]->turns.load(),
                      (long long)*turn);
    for (int i = 0; i < n && !rc; ++i) {
        golhip *h = hs[i];
        ShadowPart &p = parts[(size_t)i];
        HIP_RC(hipSetDevice(h->device));
        if (!rc) HIP_RC(hipMemsetAsync(p.d_sums, 0, 2 * sizeof(unsigned long long), h->stream));
        if (!rc) HIP_RC(hipEventRecord(p.k0, h->stream));
        if (!rc)
            HIP_RC(golk::launch_ckpt(h->cur_rows(), p.shadow, h->local_words(), (int64_t)h->row0 * h->Ww, h->il,
                                     p.d_sums, h->stream));
        if (!rc) HIP_RC(hipEventRecord(p.k1, h->stream));
        if (!rc) HIP_RC(hipStreamWaitEvent(p.side, p.k1, 0));
        if (!rc) {
            std::lock_guard<std::mutex> g(h->drain_mu);
            h->ckpt_drain = drain;
        }
    }
    return rc;
}

void shadow_kernels_wait(std::vector<ShadowPart> &parts) {
    for (auto &p : parts)
        if (p.k1 && hipSetDevice(p.device) == hipSuccess) (void)hipEventSynchronize(p.k1);
}

double shadow_stall_ms(std::vector<ShadowPart> &parts) {
    double sum = 0;
    for (auto &p : parts) {
        float ms = 0;
        if (hipSetDevice(p.device) == hipSuccess && hipEventElapsedTime(&ms, p.k0, p.k1) == hipSuccess) sum += ms;
    }
    return sum;
}

int shadow_free(std::vector<ShadowPart> &parts) {
    int rc = GOLHIP_OK;
    for (auto &p : parts) {
        HIP_RC(hipSetDevice(p.device));
        if (p.k1) HIP_RC(hipEventSynchronize(p.k1));
        if (p.side) HIP_RC(hipStreamSynchronize(p.side));
    }
    for (auto &p : parts) {
        HIP_RC(hipSetDevice(p.device));
        if (p.k0) HIP_RC(hipEventDestroy(p.k0));
        if (p.k1) HIP_RC(hipEventDestroy(p.k1));
        if (p.side && p.own_side) HIP_RC(hipStreamDestroy(p.side));
        HIP_RC(hipFree(p.shadow));
        HIP_RC(hipFree(p.d_sums));
    }
    parts.clear();
    return rc;
}

namespace {

void fill_info(const golckpt::Header &h, golhip_ckpt_info_t *info) {
    memset(info, 0, sizeof *info);
    info->width = h.width;
    info->height = h.height;
    info->turn = h.turn;
    info->alive = h.alive;
    info->hash = h.hash;
    info->file_bytes = h.file_bytes();
}

}  // namespace

}  // namespace gh

struct golhip_ckpt {
    std::string path, tmp;
    golckpt::Header hdr;
    int chunk_rows = 0;
    std::vector<gh::ShadowPart> parts;
    uint32_t *stage[2] = {nullptr, nullptr};  // page-locked
    unsigned long long *h_sums = nullptr;     // page-locked, two a part
    std::shared_ptr<gh::CkptDrain> drain = std::make_shared<gh::CkptDrain>();
    std::thread writer;
    // the writer's results
    int rc = GOLHIP_OK;
    std::string err;
    double drain_ms = 0, write_ms = 0;
};

namespace gh GOLHIP_HIDDEN {

namespace {

void set_drained(golhip_ckpt *ck) { drain_set(*ck->drain); }

// Everything the object owns on the devices (after the writer has been joined,
// or was never started).  Waits for the side streams first: they follow the
// kernels, so the shadows are no longer written.
int free_ckpt(golhip_ckpt *ck) {
    int rc = shadow_free(ck->parts);
    for (auto *s : ck->stage)
        if (s) HIP_RC(hipHostFree(s));
    if (ck->h_sums) HIP_RC(hipHostFree(ck->h_sums));
    delete ck;
    return rc;
}

// The writer thread: drains every part's shadow through the two staging
// buffers into <path>.tmp, then the header, fsync, rename.
void drain_and_write(golhip_ckpt *ck) {
    auto hip_fail = [&](const char *what, hipError_t e) {
        if (ck->rc == GOLHIP_OK) {
            ck->rc = GOLHIP_EHIP;
            ck->err = std::string("checkpoint drain: ") + what + ": " + hipGetErrorString(e);
        }
    };
    auto file_fail = [&](const char *what) {
        if (ck->rc == GOLHIP_OK) {
            ck->rc = GOLHIP_EINVAL;
            ck->err = std::string("checkpoint ") + what + " " + ck->tmp + ": " + strerror(errno);
        }
    };
    const auto t_open = Clock::now();
    const int fd = open(ck->tmp.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) file_fail("create");
    const int Ww = (int)ck->hdr.Ww;
    const size_t nparts = ck->parts.size();
    hipEvent_t staged[2] = {nullptr, nullptr};
    Clock::time_point t_first{};
    bool first = true;
    for (size_t i = 0; i < nparts && ck->rc == GOLHIP_OK; ++i) {
        ShadowPart &p = ck->parts[i];
        hipError_t e = hipSetDevice(p.device);
        for (int b = 0; b < 2 && e == hipSuccess; ++b) e = hipEventCreateWithFlags(&staged[b], hipEventDisableTiming);
        if (first) {
            t_first = Clock::now();
            first = false;
        }
        if (e == hipSuccess)
            e = hipMemcpyAsync(ck->h_sums + 2 * i, p.d_sums, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, p.side);
        // chunk k + 1 is copied while chunk k is written
        const int64_t nchunks = (p.rows + ck->chunk_rows - 1) / ck->chunk_rows;
        auto chunk_rows = [&](int64_t k) { return std::min<int64_t>(ck->chunk_rows, p.rows - k * ck->chunk_rows); };
        auto copy = [&](int64_t k) {
            return hipMemcpyAsync(ck->stage[k & 1], p.shadow + k * ck->chunk_rows * Ww, (size_t)chunk_rows(k) * Ww * 4,
                                  hipMemcpyDeviceToHost, p.side);
        };
        if (e == hipSuccess && nchunks > 0) e = copy(0);
        if (e == hipSuccess && nchunks > 0) e = hipEventRecord(staged[0], p.side);
        for (int64_t k = 0; k < nchunks && e == hipSuccess && ck->rc == GOLHIP_OK; ++k) {
            if (k + 1 < nchunks) {
                e = copy(k + 1);
                if (e == hipSuccess) e = hipEventRecord(staged[(k + 1) & 1], p.side);
            }
            if (e == hipSuccess) e = hipEventSynchronize(staged[k & 1]);
            if (e != hipSuccess) break;
            if (i + 1 == nparts && k + 1 == nchunks) ck->drain_ms = ms_since(t_first);
            const uint64_t off = golckpt::kHeaderBytes + 4ull * (uint64_t)(p.row0 + k * ck->chunk_rows) * Ww;
            if (!write_all(fd, ck->stage[k & 1], (size_t)chunk_rows(k) * Ww * 4, off)) file_fail("write");
        }
        if (e == hipSuccess) e = hipStreamSynchronize(p.side);  // (also after a file error: the staging buffers are idle)
        for (auto &ev : staged) {
            if (ev) (void)hipEventDestroy(ev);
            ev = nullptr;
        }
        if (e != hipSuccess) hip_fail("copy to the host", e);
    }
    if (ck->rc != GOLHIP_OK) {
        // the kernels still run to their end before anyone reuses or frees the shadows
        shadow_kernels_wait(ck->parts);
    }
    set_drained(ck);
    unsigned char head[golckpt::kHeaderBytes] = {};
    if (ck->rc == GOLHIP_OK) {
        for (size_t i = 0; i < nparts; ++i) {
            ck->hdr.alive += ck->h_sums[2 * i];
            ck->hdr.hash += ck->h_sums[2 * i + 1];
        }
        golckpt::encode(ck->hdr, head);
    }
    const char *what = nullptr;
    if (!file_commit(fd, ck->tmp, ck->path, head, sizeof head, ck->rc == GOLHIP_OK, &what) && what) file_fail(what);
    ck->write_ms = ms_since(t_open);
}

}  // namespace

}  // namespace gh

using namespace gh;

extern "C" {

int golhip_checkpoint_begin(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts,
                            golhip_ckpt **out) {
    if (!out) return fail(GOLHIP_EINVAL, "out is null");
    *out = nullptr;
    if (!path || !*path) return fail(GOLHIP_EINVAL, "path is empty");
    if (int rc = group_check(hs, n)) return rc;
    for (int i = 0; i < n; ++i)
        if (hs[i]->ringed()) return fail(GOLHIP_EINVAL, "checkpoint of a ringed handle: the ranks of a ring would have "
                                                        "to agree on the turn (not supported)");
    int chunk = 0;
    if (int rc = chunk_rows_for(opts, 4ll * hs[0]->Ww, &chunk)) return rc;
    // an earlier checkpoint (or image) of these handles leaves the device first
    drain_wait_earlier(hs, n);
    golhip_ckpt *ck = new golhip_ckpt();
    ck->path = path;
    ck->tmp = ck->path + ".tmp";
    ck->hdr.width = hs[0]->W;
    ck->hdr.height = hs[0]->H;
    ck->hdr.Ww = (uint32_t)hs[0]->Ww;
    int max_rows = 0;
    // everything is allocated before a mutex is taken
    int rc = shadow_alloc(hs, n, "checkpoint", ck->parts, &max_rows);
    ck->chunk_rows = std::min(chunk, std::max(1, max_rows));
    const size_t stage_bytes = (size_t)ck->chunk_rows * hs[0]->Ww * 4;
    // (portable: the side stream of every strip's device copies into them)
    for (int b = 0; b < 2 && !rc; ++b)
        if (hipHostMalloc((void **)&ck->stage[b], stage_bytes, hipHostMallocPortable) != hipSuccess)
            rc = fail(GOLHIP_ENOMEM, "checkpoint staging buffer of %zu bytes", stage_bytes);
    if (!rc) HIP_RC(hipHostMalloc((void **)&ck->h_sums, (size_t)n * 2 * sizeof(unsigned long long), hipHostMallocPortable));
    if (!rc) rc = shadow_enqueue(hs, n, ck->parts, ck->drain, &ck->hdr.turn);
    if (rc) {
        // (whatever was enqueued finishes first: free_ckpt waits for the events and side streams)
        const std::string msg = golhip_last_error();
        set_drained(ck);
        (void)free_ckpt(ck);
        return fail(rc, "%s", msg.c_str());
    }
    ck->writer = std::thread(drain_and_write, ck);
    *out = ck;
    return GOLHIP_OK;
}

int golhip_drain_wait(golhip_t *hs, int32_t n) {
    if (int rc = group_check(hs, n, false)) return rc;
    drain_wait_earlier(hs, n);
    return GOLHIP_OK;
}

int golhip_checkpoint_wait(golhip_ckpt *ck, golhip_ckpt_info_t *info) {
    if (!ck) return fail(GOLHIP_EINVAL, "null checkpoint");
    if (ck->writer.joinable()) ck->writer.join();
    int rc = ck->rc;
    const std::string err = ck->err;
    if (info) {
        fill_info(ck->hdr, info);
        info->drain_ms = ck->drain_ms;
        info->write_ms = ck->write_ms;
        if (rc == GOLHIP_OK) info->stall_ms = shadow_stall_ms(ck->parts);
    }
    const int frc = free_ckpt(ck);
    if (rc) return fail(rc, "%s", err.c_str());
    return frc;
}

int golhip_checkpoint_info(const char *path, golhip_ckpt_info_t *info) {
    if (!path || !info) return fail(GOLHIP_EINVAL, "null argument");
    golckpt::Header h;
    std::string why;
    switch (golckpt::read_info(path, &h, &why)) {
    case 0: break;
    case 1: return fail(GOLHIP_EINVAL, "checkpoint: %s", why.c_str());
    default: return fail(GOLHIP_ECORRUPT, "checkpoint %s: %s", path, why.c_str());
    }
    fill_info(h, info);
    return GOLHIP_OK;
}

int golhip_checkpoint_load(golhip_t *hs, int32_t n, const char *path, const golhip_ckpt_opts_t *opts,
                           golhip_ckpt_info_t *info) {
    if (!path) return fail(GOLHIP_EINVAL, "path is null");
    if (int rc = group_check(hs, n, false)) return rc;
    golhip_ckpt_info_t fi;
    if (int rc = golhip_checkpoint_info(path, &fi)) return rc;
    if (fi.width != hs[0]->W || fi.height != hs[0]->H)
        return fail(GOLHIP_EINVAL, "checkpoint %s holds a %d x %d board, the handles a %d x %d one", path, fi.width,
                    fi.height, hs[0]->W, hs[0]->H);
    int chunk = 0;
    if (int rc = chunk_rows_for(opts, 4ll * hs[0]->Ww, &chunk)) return rc;
    int max_rows = 0;
    for (int i = 0; i < n; ++i) max_rows = std::max(max_rows, hs[i]->rows);
    chunk = std::min(chunk, std::max(1, max_rows));
    const int Ww = hs[0]->Ww;

    std::vector<std::unique_lock<std::mutex>> locks;
    for (int i = 0; i < n; ++i) locks.emplace_back(hs[i]->mu);
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return fail(GOLHIP_EINVAL, "checkpoint: open %s: %s", path, strerror(errno));
    uint32_t *stage[2] = {nullptr, nullptr};
    int rc = GOLHIP_OK;
    HIP_RC(hipSetDevice(hs[0]->device));
    for (int b = 0; b < 2 && !rc; ++b)
        if (hipHostMalloc((void **)&stage[b], (size_t)chunk * Ww * 4, hipHostMallocPortable) != hipSuccess)
            rc = fail(GOLHIP_ENOMEM, "checkpoint staging buffer of %zu bytes", (size_t)chunk * Ww * 4);
    uint64_t alive = 0, hash = 0;
    for (int i = 0; i < n && !rc; ++i) {
        golhip *h = hs[i];
        HIP_RC(hipSetDevice(h->device));
        hipEvent_t used[2] = {nullptr, nullptr};
        for (int b = 0; b < 2 && !rc; ++b) HIP_RC(hipEventCreateWithFlags(&used[b], hipEventDisableTiming));
        // the canonical words land in the other board buffer; the kernel stores the rows from there
        uint32_t *canon = h->prev_rows();
        int64_t k = 0;
        for (int64_t r = 0; r < h->rows && !rc; r += chunk, ++k) {
            const int64_t nr = std::min<int64_t>(chunk, h->rows - r);
            const int b = (int)(k & 1);
            if (k >= 2) HIP_RC(hipEventSynchronize(used[b]));
            if (!rc && !read_all(fd, stage[b], (size_t)nr * Ww * 4, golckpt::kHeaderBytes + 4ull * (uint64_t)(h->row0 + r) * Ww))
                rc = fail(GOLHIP_ECORRUPT, "checkpoint %s: file size: rows %lld.. cannot be read", path,
                          (long long)(h->row0 + r));
            if (!rc) HIP_RC(hipMemcpyAsync(canon + r * Ww, stage[b], (size_t)nr * Ww * 4, hipMemcpyHostToDevice, h->stream));
            if (!rc) HIP_RC(hipEventRecord(used[b], h->stream));
        }
        const int il = want_il(h);
        if (!rc) HIP_RC(hipMemsetAsync(h->d_scalars + 2, 0, 2 * sizeof(unsigned long long), h->stream));
        if (!rc)
            HIP_RC(golk::launch_ckpt_load(canon, h->cur_rows(), h->local_words(), (int64_t)h->row0 * Ww, h->W, Ww, il,
                                          h->d_scalars + 2, h->stream));
        if (!rc)
            HIP_RC(hipMemcpyAsync(h->h_scalars + 2, h->d_scalars + 2, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost,
                                  h->stream));
        // (also after an error: the staging buffers are idle before they are freed)
        if (int src = sync_stream(h); src && !rc) rc = src;
        for (auto ev : used)
            if (ev) (void)hipEventDestroy(ev);
        if (rc) break;
        h->il = il;
        h->loaded = true;
        h->turns = fi.turn;
        h->alive_turn = -1;
        h->flips_valid = false;
        h->ft_est = 0;  // a new board (as loaded_canonical)
        h->group_ft_est = 0;
        alive += h->h_scalars[2];
        hash += h->h_scalars[3];
    }
    close(fd);
    for (auto *s : stage)
        if (s) (void)hipHostFree(s);
    if (rc) return rc;
    if (alive != fi.alive)
        return fail(GOLHIP_ECORRUPT, "checkpoint %s: alive count: the payload holds %llu cells, the header says %llu", path,
                    (unsigned long long)alive, (unsigned long long)fi.alive);
    if (hash != fi.hash)
        return fail(GOLHIP_ECORRUPT, "checkpoint %s: digest: the payload's is %016llx, the header says %016llx", path,
                    (unsigned long long)hash, (unsigned long long)fi.hash);
    if (info) *info = fi;
    return GOLHIP_OK;
}

}  // extern "C"
