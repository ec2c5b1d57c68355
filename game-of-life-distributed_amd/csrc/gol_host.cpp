// gol_host.cpp — the reference's gol.Run host flow over libgolhip.so.
//
// Mirrors gol/distributor.go:30-209 (distributor), :223-280 (keyPress),
// :283-302 (ticker) and gol/io.go:42-126 (PGM io).  The turn loop itself is
// golhip_step; everything here is event sequencing and file I/O.
#include "gol_host.h"

#include <sys/stat.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <thread>

#include "../../include/golhip.h"
#include "../../include/golrun.h"
#include "gol_image_file.h"

namespace gol {

std::string StateString(State s) {
    switch (s) {
        case State::Paused: return "Paused";
        case State::Executing: return "Executing";
        case State::Quitting: return "Quitting";
    }
    return "Incorrect State";
}

std::string Event::String() const {
    switch (kind) {
        case EventKind::AliveCellsCount: return "Alive Cells " + std::to_string(CellsCount);
        case EventKind::ImageOutputComplete: return "File " + Filename + " output complete";
        case EventKind::StateChange: return StateString(NewState);
        default: return "";  // CellFlipped, TurnComplete, FinalTurnComplete (event.go:107-129)
    }
}

RunOptions::Pattern ParsePattern(const std::string &spec) {
    auto bad = [&](const char *what) {
        return std::runtime_error("pattern \"" + spec + "\": " + what + " (expected path@x,y[,op], op one of copy|or|xor|clear)");
    };
    const size_t at = spec.rfind('@');
    if (at == std::string::npos || at == 0) throw bad("no path@");
    RunOptions::Pattern p;
    p.path = spec.substr(0, at);
    std::vector<std::string> f;
    std::stringstream ss(spec.substr(at + 1));
    for (std::string t; std::getline(ss, t, ',');) f.push_back(t);
    if (f.size() < 2 || f.size() > 3) throw bad("bad position");
    int64_t *out[2] = {&p.x, &p.y};
    for (int i = 0; i < 2; ++i) {
        char *end = nullptr;
        const long long v = std::strtoll(f[i].c_str(), &end, 10);
        if (f[i].empty() || *end) throw bad("bad position");
        *out[i] = v;
    }
    if (f.size() == 3) {
        static const char *const names[] = {"copy", "or", "xor", "clear"};
        p.op = -1;
        for (int i = 0; i < 4; ++i)
            if (f[2] == names[i]) p.op = i;
        if (p.op < 0) throw bad("unknown op");
    }
    return p;
}

// ---------------------------------------------------------------- PGM io
// readPgmImage (io.go:90-126): whitespace-separated fields P5, W, H, 255;
// the raster follows the single whitespace byte after maxval.
std::vector<uint8_t> ReadPgm(const std::string &path, int64_t width, int64_t height) {
    std::ifstream f(path, std::ios::binary);
    if (!f) throw std::runtime_error("open " + path + ": no such file or directory");
    std::vector<uint8_t> data((std::istreambuf_iterator<char>(f)), std::istreambuf_iterator<char>());
    size_t pos = 0;
    auto ws = [](uint8_t c) { return c == ' ' || c == '\t' || c == '\n' || c == '\r' || c == '\v' || c == '\f'; };
    std::string fields[4];
    for (auto &fld : fields) {
        while (pos < data.size() && ws(data[pos])) ++pos;
        while (pos < data.size() && !ws(data[pos])) fld.push_back((char)data[pos++]);
    }
    ++pos;
    if (fields[0] != "P5") throw std::runtime_error("Not a pgm file");
    if (std::atoll(fields[1].c_str()) != width) throw std::runtime_error("Incorrect width");
    if (std::atoll(fields[2].c_str()) != height) throw std::runtime_error("Incorrect height");
    if (std::atoll(fields[3].c_str()) != 255) throw std::runtime_error("Incorrect maxval/bit depth");
    const size_t n = (size_t)width * height;
    if (data.size() < pos + n) throw std::runtime_error("short raster in " + path);
    return std::vector<uint8_t>(data.begin() + pos, data.begin() + pos + n);
}

// writePgmImage (io.go:42-87): "P5\n" W " " H "\n" "255\n" + raster, one bulk write.
void WritePgm(const std::string &path, int64_t width, int64_t height, const uint8_t *raster) {
    std::ofstream f(path, std::ios::binary | std::ios::trunc);
    if (!f) throw std::runtime_error("create " + path + " failed");
    f << "P5\n" << width << " " << height << "\n" << 255 << "\n";
    f.write(reinterpret_cast<const char *>(raster), (std::streamsize)width * height);
    f.flush();
    if (!f) throw std::runtime_error("write " + path + " failed");
}

namespace {

void check(int rc) {
    if (rc != GOLHIP_OK) throw std::runtime_error(std::string("golhip: ") + golhip_last_error());
}

int env_int(const char *name, int dflt) {
    const char *v = std::getenv(name);
    return (v && *v) ? std::atoi(v) : dflt;
}

// The board behind Run: one whole-torus handle, or row strips (GOL_NGPU /
// GOL_STRIPS) stepped together by golhip_group_step_ex.  Every side channel
// of the strips is gathered in strip order, which is the board's row-major
// order: alive lists and flip lists concatenate, counts add up.
// Page-locked flip-list buffer the engine's flip kernel writes directly
// (golhip_host_alloc): 4-byte cell indices y * W + x.
struct FlipBuffer {
    uint32_t *p = nullptr;
    uint64_t cap = 0;  // entries
    // at least n entries (contents are not kept)
    void grow(uint64_t n) {
        if (n <= cap) return;
        void *q = nullptr;
        check(golhip_host_alloc(n * sizeof(uint32_t), &q));
        if (p) golhip_host_free(p);
        p = static_cast<uint32_t *>(q);
        cap = n;
    }
    ~FlipBuffer() {
        if (p) golhip_host_free(p);
    }
};

// Page-locked frames of the live view, written by the view kernel itself: two
// halves of `per_half` frames, so the frame a consumer may be copying (the
// last one published, in the half of the previous batch) is never the one the
// device writes.  At most kViewRingBytes in all.
constexpr uint64_t kViewRingBytes = 64ull << 20;
struct ViewRing {
    uint8_t *p = nullptr;
    uint64_t frame_bytes = 0;
    int64_t per_half = 0;
    int half = 0;  // the half the next batch writes
    ViewRing(const golhip_view_t &v, int64_t batch_frames) {
        frame_bytes = (uint64_t)v.out_w * (uint64_t)v.out_h * (v.format == GOLHIP_VIEW_GRAY8 ? 1u : 4u);
        if (frame_bytes == 0 || 2 * frame_bytes > kViewRingBytes)
            throw std::runtime_error("live view: a frame of " + std::to_string(frame_bytes) +
                                     " bytes does not fit the 64 MiB frame ring twice");
        per_half = std::max<int64_t>(1, std::min<int64_t>(batch_frames, (int64_t)(kViewRingBytes / 2 / frame_bytes)));
        void *q = nullptr;
        check(golhip_host_alloc(2 * (uint64_t)per_half * frame_bytes, &q));
        p = static_cast<uint8_t *>(q);
    }
    uint8_t *slot(int h, int64_t i) const { return p + ((uint64_t)h * per_half + (uint64_t)i) * frame_bytes; }
    ~ViewRing() {
        if (p) golhip_host_free(p);
    }
};

struct Engine {
    std::vector<golhip_t> hs;
    std::vector<int64_t> row0;
    int64_t W = 0, H = 0;
    Engine(int64_t w, int64_t hgt, const RunOptions &opt) : W(w), H(hgt) {
        const int ngpu = opt.ngpu >= 0 ? opt.ngpu : env_int("GOL_NGPU", 1);
        const int strips = opt.strips >= 0 ? opt.strips : env_int("GOL_STRIPS", 0);
        int n = strips > 0 ? strips : std::max(1, ngpu);
        n = (int)std::min<int64_t>(n, hgt);
        const bool view_strips = opt.view_strips >= 0 ? opt.view_strips != 0 : env_int("GOL_VIEW_STRIPS", 0) != 0;
        if (n > 1 && opt.view.scale > 0 && !view_strips)
            throw std::runtime_error("live view: a run of " + std::to_string(n) +
                                     " strips (GOL_STRIPS / GOL_NGPU) has no view; run it on one strip"
                                     " (or opt in: RunOptions::view_strips, GOL_VIEW_STRIPS=1)");
        if (n <= 1) {
            hs.push_back(nullptr);
            row0.push_back(0);
            check(golhip_create((int32_t)w, (int32_t)hgt, opt.device, 0, &hs[0]));
            set_rule(opt);
            return;
        }
        int32_t ndev = 0;
        check(golhip_device_count(&ndev));
        const int devs = std::max(1, std::min(ngpu > 0 ? ngpu : 1, (int)ndev));
        for (int i = 0; i < n; ++i) {
            const int64_t r0 = hgt * i / n, r1 = hgt * (i + 1) / n;
            golhip_t h = nullptr;
            const int dev = devs > 1 ? i % devs : opt.device;
            const int rc = golhip_create_strip((int32_t)w, (int32_t)hgt, (int32_t)r0, (int32_t)(r1 - r0), dev, 0, &h);
            if (rc != GOLHIP_OK) {
                for (golhip_t x : hs) golhip_destroy(x);
                hs.clear();
                check(rc);
            }
            hs.push_back(h);
            row0.push_back(r0);
        }
        set_rule(opt);
    }
    // RunOptions::rule on every handle, before a board is there; right after it RunOptions::rule_flips and ::plane
    void set_rule(const RunOptions &opt) {
        const bool fused = opt.rule_flips >= 0 ? opt.rule_flips != 0 : env_int("GOL_RULE_FLIPS", 0) != 0;
        const bool plane = opt.plane >= 0 ? opt.plane != 0 : env_int("GOL_PLANE", 0) != 0;
        for (golhip_t h : hs) {
            check(golhip_set_rule(h, opt.rule.birth, opt.rule.survive));
            check(golhip_set_rule_flips(h, fused ? 1 : 0));
            check(golhip_set_topology(h, plane ? GOLHIP_TOPOLOGY_PLANE : GOLHIP_TOPOLOGY_TORUS));
        }
    }
    ~Engine() {
        if (ckpt) golhip_checkpoint_wait(ckpt, nullptr);
        for (golhip_t h : hs) golhip_destroy(h);
    }
    // The checkpoint in flight (RunOptions::checkpoint_path): at most one.
    golhip_ckpt *ckpt = nullptr;
    int64_t ckpt_turn = -1;  // turn of the last checkpoint begun
    void ckpt_wait() {
        if (!ckpt) return;
        golhip_ckpt *c = ckpt;
        ckpt = nullptr;
        check(golhip_checkpoint_wait(c, nullptr));
    }
    void ckpt_begin(const std::string &path, int64_t turn) {
        ckpt_wait();
        check(golhip_checkpoint_begin(hs.data(), (int32_t)hs.size(), path.c_str(), nullptr, &ckpt));
        ckpt_turn = turn;
    }
    // board and turn from a checkpoint file (RunOptions::resume_path)
    void resume(const std::string &path) {
        check(golhip_checkpoint_load(hs.data(), (int32_t)hs.size(), path.c_str(), nullptr, nullptr));
    }
    // streamed images (RunOptions::stream_images): golhip_image_begin of the whole board
    golhip_image *image_begin(const std::string &path) {
        golhip_image *im = nullptr;
        check(golhip_image_begin(hs.data(), (int32_t)hs.size(), path.c_str(), nullptr, &im));
        return im;
    }
    // the streamed load; a failure carries ReadPgm's message
    void load_image(const std::string &path) {
        if (golhip_image_load(hs.data(), (int32_t)hs.size(), path.c_str(), nullptr, nullptr) != GOLHIP_OK)
            throw std::runtime_error(golhip_last_error());
    }
    // An earlier image or checkpoint of the board has left the device: a begin that follows does not
    // wait for it inside the call (callers begin under the run's mutex and wait here first, off it).
    void drain_wait() { check(golhip_drain_wait(hs.data(), (int32_t)hs.size())); }
    bool one() const { return hs.size() == 1; }
    int64_t rows(size_t i) const { return (i + 1 < row0.size() ? row0[i + 1] : H) - row0[i]; }
    void load(const uint8_t *raster) {
        for (size_t i = 0; i < hs.size(); ++i) check(golhip_load_bytes(hs[i], raster + row0[i] * W));
    }
    // patterns (RunOptions::blank, patterns): an empty board; a pattern file on the whole board
    void clear() {
        for (golhip_t h : hs) check(golhip_clear(h));
    }
    void stamp(const RunOptions::Pattern &p) {
        if (golhip_stamp_file(hs.data(), (int32_t)hs.size(), p.path.c_str(), (int32_t)p.x, (int32_t)p.y, p.op, nullptr) !=
            GOLHIP_OK)
            throw std::runtime_error(golhip_last_error());
    }
    void snapshot(uint8_t *out) {
        for (size_t i = 0; i < hs.size(); ++i) check(golhip_snapshot_bytes(hs[i], out + row0[i] * W));
    }
    void alive_count(uint64_t *n, int64_t *at) {
        *n = 0;
        for (golhip_t h : hs) {
            uint64_t c = 0;
            check(golhip_alive_count(h, &c, at));
            *n += c;
        }
    }
    // calculateAliveCells (distributor.go:420-432) / the flips of the last turn
    std::vector<util::Cell> cells(int (*fn)(golhip_t, int32_t *, uint64_t, uint64_t *), bool transpose) {
        std::vector<util::Cell> out;
        for (golhip_t h : hs) {
            uint64_t n = 0;
            int rc = fn(h, nullptr, 0, &n);
            if (rc != GOLHIP_OK && rc != GOLHIP_ERANGE) check(rc);
            std::vector<int32_t> xy(2 * std::max<uint64_t>(n, 1));
            check(fn(h, xy.data(), n, &n));
            for (uint64_t i = 0; i < n; ++i) {
                util::Cell c;
                c.X = transpose ? xy[2 * i + 1] : xy[2 * i];
                c.Y = transpose ? xy[2 * i] : xy[2 * i + 1];
                out.push_back(c);
            }
        }
        return out;
    }
    void step(int64_t turns) {
        if (one()) {
            check(golhip_step(hs[0], turns, 0));
            check(golhip_sync(hs[0]));
        } else {
            check(golhip_group_step_ex(hs.data(), (int32_t)hs.size(), turns, 0));
        }
    }
    // Up to `want` turns with every turn's flip list as cell indices y * W + x
    // (golhip_flip_stream's contract: stops before a turn that does not fit;
    // GOLHIP_ERANGE with *n = what the first turn needs).  Strips: the same
    // contract on the whole board (golhip_group_flip_stream).
    int flip_stream(int64_t want, FlipBuffer &fb, uint64_t *counts, int64_t *done, uint64_t *n) {
        if (one()) return golhip_flip_stream(hs[0], want, GOLHIP_FLIPS_INDEX, fb.p, fb.cap, counts, done, n);
        return golhip_group_flip_stream(hs.data(), (int32_t)hs.size(), want, GOLHIP_FLIPS_INDEX, fb.p, fb.cap, counts, done,
                                        n);
    }
};

}  // namespace

void Run(Params p, Chan<Event> *events, Chan<char32_t> *keyPresses, const RunOptions &opt) {
    const int64_t W = p.ImageWidth, H = p.ImageHeight;
    if (W <= 0 || H <= 0 || W > INT32_MAX || H > INT32_MAX || p.Turns < 0) throw std::runtime_error("bad Params");
    const std::string name = std::to_string(W) + "x" + std::to_string(H);
    const bool quirks = opt.ref_quirks;

    const bool ckpt_on = !opt.checkpoint_path.empty();
    if (opt.checkpoint_every < 0 || (opt.checkpoint_every > 0 && !ckpt_on))
        throw std::runtime_error("checkpoint_every must be >= 0 and needs checkpoint_path");
    const bool stream = opt.stream_images >= 0 ? opt.stream_images != 0 : env_int("GOL_STREAM_IMAGES", 0) != 0;
    if (opt.image_every < 0 || (opt.image_every > 0 && !stream))
        throw std::runtime_error("image_every must be >= 0 and needs stream_images");

    // distributor.go:39-41 -> io.readPgmImage; a resumed run takes board and
    // turn from its checkpoint instead (and fails where readPgmImage fails)
    int64_t T0 = 0;
    std::vector<uint8_t> raster;
    const std::string image_path = opt.root + "/images/" + name + ".pgm";
    if (!opt.resume_path.empty() && (opt.blank || !opt.patterns.empty()))
        throw std::runtime_error("resume: a run from a checkpoint takes neither blank nor patterns (a restarted job "
                                 "must not stamp twice)");
    if (opt.rule.birth > 0x1FF || opt.rule.survive > 0x1FF) throw std::runtime_error("rule masks above 0x1FF");
    const bool conway = opt.rule.birth == 0x008 && opt.rule.survive == 0x00C;
    // every pattern file's checks before a device is touched (golhip_pattern_info needs none)
    for (const RunOptions::Pattern &ps : opt.patterns) {
        golhip_pattern_info_t pi{};
        if (!conway) {
            // golhip_pattern_info takes Conway's files alone: a run on another rule checks the file's
            // rule here (its own or none; an explicit B3/S23, and the size, are golhip_stamp_file's to refuse)
            uint32_t fb = 0, fs = 0;
            if (golhip_pattern_rule(ps.path.c_str(), &fb, &fs) != GOLHIP_OK) throw std::runtime_error(golhip_last_error());
            if (!(fb == opt.rule.birth && fs == opt.rule.survive) && !(fb == 0x008 && fs == 0x00C)) {
                char file_rule[32] = "", run_rule[32] = "";
                golhip_rule_format(fb, fs, file_rule, sizeof file_rule);
                golhip_rule_format(opt.rule.birth, opt.rule.survive, run_rule, sizeof run_rule);
                throw std::runtime_error("RLE: rule " + std::string(file_rule) + " is not the board's " + run_rule);
            }
        } else if (golhip_pattern_info(ps.path.c_str(), &pi) != GOLHIP_OK) {
            throw std::runtime_error(golhip_last_error());
        }
        if (pi.width > W || pi.height > H)
            throw std::runtime_error("pattern " + ps.path + " is " + std::to_string(pi.width) + " x " +
                                     std::to_string(pi.height) + ": it does not fit the " + name + " board");
        if (ps.x < 0 || ps.x >= W || ps.y < 0 || ps.y >= H)
            throw std::runtime_error("pattern " + ps.path + ": corner (" + std::to_string(ps.x) + ", " +
                                     std::to_string(ps.y) + ") is not on the " + name + " board");
    }
    if (opt.blank) {
        // no image: the board starts empty (golhip_clear below)
    } else if (opt.resume_path.empty() && stream) {
        // the header's checks before a device is touched, against this run's board so that they come in
        // ReadPgm's order (golhip_image_info has no board: its size checks would come too late); the
        // raster follows below, chunk by chunk, behind the same checks in golhip_image_load
        golimg::Info fi;
        std::string why;
        if (!golimg::read_info(image_path.c_str(), W, H, &fi, &why)) throw std::runtime_error(why);
    } else if (opt.resume_path.empty()) {
        raster = ReadPgm(image_path, W, H);
        std::printf("File %s input done!\n", name.c_str());
        std::fflush(stdout);
    } else {
        golhip_ckpt_info_t ci;
        check(golhip_checkpoint_info(opt.resume_path.c_str(), &ci));
        if (ci.width != W) throw std::runtime_error("Incorrect width");
        if (ci.height != H) throw std::runtime_error("Incorrect height");
        if (ci.turn > p.Turns)
            throw std::runtime_error("checkpoint " + opt.resume_path + " is at turn " + std::to_string(ci.turn) +
                                     ", past the run's " + std::to_string(p.Turns) + " turns");
        T0 = ci.turn;
    }

    Engine board(W, H, opt);
    if (opt.blank) {
        board.clear();
    } else if (opt.resume_path.empty() && stream) {
        board.load_image(image_path);
        std::printf("File %s input done!\n", name.c_str());
        std::fflush(stdout);
    } else if (opt.resume_path.empty()) {
        board.load(raster.data());
    } else {
        board.resume(opt.resume_path);
        std::printf("Checkpoint %s input done! (turn %lld)\n", opt.resume_path.c_str(), (long long)T0);
        std::fflush(stdout);
    }
    std::vector<uint8_t>().swap(raster);
    for (const RunOptions::Pattern &ps : opt.patterns) board.stamp(ps);

    // Live view: frames land in the ring and are published by pointer.  With
    // cell events the turns keep the flip stream, in batches that end on the
    // frame turns, and golhip_view_frame renders between them; without, the
    // batch itself is golhip_view_stream.  On row strips (view_strips) both
    // are the group calls, which on one whole-torus handle are the same calls.
    const bool view_on = opt.view.scale > 0;
    if (view_on && (!opt.view_sink || opt.view_every < 1)) throw std::runtime_error("live view: no sink, or every < 1");
    const int64_t batch_turns = opt.batch_turns > 0 ? opt.batch_turns : (opt.cell_events ? 64 : 256);
    std::unique_ptr<ViewRing> ring;
    if (view_on) ring.reset(new ViewRing(opt.view, opt.cell_events ? 1 : std::max<int64_t>(1, batch_turns / opt.view_every)));
    // the current board's frame into the ring's next half, published at once
    auto view_now = [&] {
        int64_t at = 0;
        uint8_t *f = ring->slot(ring->half, 0);
        check(golhip_group_view_frame(board.hs.data(), (int32_t)board.hs.size(), &opt.view, f, ring->frame_bytes, &at));
        opt.view_sink->publish(f, ring->frame_bytes, at);
        ring->half ^= 1;
    };
    struct KeepLastFrame {  // the sink outlives the ring
        ViewSink *s;
        ~KeepLastFrame() {
            if (s) s->keep_copy();
        }
    } keep_last{view_on ? opt.view_sink : nullptr};
    if (view_on) view_now();  // turn 0, before the first event

    auto send = [&](Event e) {
        if (events) events->send(std::move(e));
    };
    auto write_snapshot = [&](int64_t turn, bool transposed) -> std::string {
        std::vector<uint8_t> snap((size_t)W * H);
        board.snapshot(snap.data());
        if (transposed) {  // the reference streams (*world)[x][y] for s/q (distributor.go:234-238)
            std::vector<uint8_t> t((size_t)W * H);
            for (int64_t y = 0; y < H; ++y)
                for (int64_t x = 0; x < W; ++x) t[(size_t)x * H + y] = snap[(size_t)y * W + x];
            snap.swap(t);
        }
        const std::string fname = name + "x" + std::to_string(turn);
        mkdir((opt.root + "/out").c_str(), 0777);  // io.go:43 os.Mkdir("out")
        WritePgm(opt.root + "/out/" + fname + ".pgm", W, H, snap.data());
        std::printf("File %s output done!\n", fname.c_str());
        std::fflush(stdout);
        return fname;
    };

    // RunOptions::save_rle: the alive box of the board as out/<W>x<H>x<turn>.rle,
    // written at a turn boundary (the caller holds `mu`, or no turn is running)
    // before the image of that turn is begun, so before its ImageOutputComplete.
    const bool save_rle = opt.save_rle >= 0 ? opt.save_rle != 0 : env_int("GOL_SAVE_RLE", 0) != 0;
    auto write_rle = [&](int64_t turn) {
        if (!save_rle) return;
        const std::string fname = name + "x" + std::to_string(turn) + ".rle";
        mkdir((opt.root + "/out").c_str(), 0777);
        const int rc = golhip_save_rle(board.hs.data(), (int32_t)board.hs.size(), (opt.root + "/out/" + fname).c_str(), 0, 0, 0,
                                       0, 0, nullptr);
        if (rc == GOLHIP_EINVAL && std::string(golhip_last_error()) == "board is empty") {
            std::printf("File %s not written: the board is empty\n", fname.c_str());
        } else {
            check(rc);
            std::printf("File %s output done!\n", fname.c_str());
        }
        std::fflush(stdout);
    };

    // Streamed: the image is begun at a turn boundary (the caller holds `mu`,
    // or no turn is running) and waited for off it; the file, the line and the
    // event are write_snapshot's.
    // One image of the run in flight at a time, whoever began it (the key
    // thread, the periodic images): two writers of one turn would share a path
    // and its .tmp.  Taken before `mu` and the begin, given back when the file
    // is complete, possibly by another thread.
    struct ImageSlot {
        std::mutex m;
        std::condition_variable cv;
        bool busy = false;
        void acquire() {
            std::unique_lock<std::mutex> lk(m);
            cv.wait(lk, [&] { return !busy; });
            busy = true;
        }
        void release() {
            {
                std::lock_guard<std::mutex> lk(m);
                busy = false;
            }
            cv.notify_all();
        }
    } image_slot;
    struct SlotRelease {
        ImageSlot *s;
        ~SlotRelease() {
            if (s) s->release();
        }
    };
    auto image_name = [&](int64_t turn) { return name + "x" + std::to_string(turn); };
    auto image_begin = [&](int64_t turn) {
        mkdir((opt.root + "/out").c_str(), 0777);  // io.go:43 os.Mkdir("out")
        return board.image_begin(opt.root + "/out/" + image_name(turn) + ".pgm");
    };
    auto image_finish = [&](golhip_image *im, int64_t turn) {
        check(golhip_image_wait(im, nullptr));
        std::printf("File %s output done!\n", image_name(turn).c_str());
        std::fflush(stdout);
        Event e;
        e.kind = EventKind::ImageOutputComplete;
        e.CompletedTurns = turn;
        e.Filename = image_name(turn);
        send(e);
    };

    // distributor.go:72-80: CellFlipped for every cell alive at load, turn 0
    // (a resumed run: the checkpoint's board, at its turn).
    if (opt.cell_events && events)
        for (const util::Cell &c : board.cells(golhip_alive_cells, quirks)) {
            Event e;
            e.kind = EventKind::CellFlipped;
            e.CompletedTurns = T0;
            e.Cell = c;
            send(e);
        }

    std::mutex mu;                 // the reference's `mu`: held by the turn loop and by pause
    std::atomic<int> waiters{0};   // helpers queued for `mu` (std::mutex is not fair)
    std::atomic<int64_t> turn{T0};  // completed turns
    // helpers take `mu` through this, so the turn loop can step aside for them
    auto lock_mu = [&]() {
        ++waiters;
        std::unique_lock<std::mutex> g(mu);
        --waiters;
        return g;
    };
    std::atomic<bool> finished{false}, quit{false};
    std::mutex tick_mu;
    std::condition_variable tick_cv;

    // ticker (distributor.go:283-302): (turn, count) read as one pair from the engine.
    std::exception_ptr helper_err;  // first exception raised on a helper thread
    std::mutex err_mu;
    auto guarded = [&](auto body) {
        return [&, body] {
            try {
                body();
            } catch (...) {
                std::lock_guard<std::mutex> g(err_mu);
                if (!helper_err) helper_err = std::current_exception();
                quit = true;
            }
        };
    };
    std::thread ticker(guarded([&] {
        const auto period = std::chrono::duration<double>(opt.ticker_seconds);
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(tick_mu);
                if (tick_cv.wait_for(lk, period, [&] { return finished.load(); })) break;
            }
            uint64_t n = 0;
            int64_t at = 0;
            {
                auto g = lock_mu();  // blocked while paused, like the reference
                board.alive_count(&n, &at);
            }
            Event e;
            e.kind = EventKind::AliveCellsCount;
            e.CompletedTurns = at;
            e.CellsCount = (int64_t)n;
            send(e);
        }
    }));

    // keyPress (distributor.go:223-280); a nil channel simply never delivers.
    std::thread keys;
    if (keyPresses) keys = std::thread(guarded([&] {
        char32_t k;
        while (!finished.load()) {
            int r = keyPresses->try_recv(k);
            if (r < 0) break;
            if (r == 0) {
                std::this_thread::sleep_for(std::chrono::milliseconds(2));
                continue;
            }
            if (k == U's' || k == U'q') {
                std::string fname;
                int64_t t;
                golhip_image *im = nullptr;
                const bool streamed_key = stream && !quirks;
                SlotRelease slot{nullptr};
                if (streamed_key) {
                    // off `mu`: a periodic image in flight finishes its file, and an earlier job's shadow drains
                    image_slot.acquire();
                    slot.s = &image_slot;
                    board.drain_wait();
                }
                {
                    auto g = lock_mu();  // snapshot at a turn boundary
                    t = turn.load();
                    write_rle(t);
                    // streamed: only the enqueue holds `mu`; the turn loop steps on while the file is written
                    if (streamed_key) im = image_begin(t);
                    else fname = write_snapshot(t, quirks);
                    // with checkpointing on, the turn loop sees it before its next call: the
                    // run stops at the snapshot's turn, the turn of the take-over checkpoint
                    // (without, `q` is raised after the event below, as it always was)
                    if (k == U'q' && ckpt_on) quit = true;
                }
                if (im) {
                    image_finish(im, t);
                } else {
                    Event e;
                    e.kind = EventKind::ImageOutputComplete;
                    e.CompletedTurns = t;
                    e.Filename = fname;
                    send(e);
                }
                if (k == U'q') {
                    quit = true;
                    break;
                }
            } else if (k == U'p') {
                auto g = lock_mu();
                std::printf("%lld\n", (long long)turn.load());
                std::fflush(stdout);
                if (!quirks) {
                    Event e;
                    e.kind = EventKind::StateChange;
                    e.CompletedTurns = turn.load();
                    e.NewState = State::Paused;
                    send(e);
                }
                char32_t k2 = 0;
                while (!finished.load()) {
                    int r2 = keyPresses->try_recv(k2);
                    if (r2 < 0) break;
                    if (r2 == 1 && k2 == U'p') break;
                    std::this_thread::sleep_for(std::chrono::milliseconds(2));
                }
                std::printf("Continuing\n");
                std::fflush(stdout);
                if (!quirks) {
                    Event e;
                    e.kind = EventKind::StateChange;
                    e.CompletedTurns = turn.load();
                    e.NewState = State::Executing;
                    send(e);
                }
            }
        }
    }));

    // The periodic image in flight (RunOptions::image_every): at most one.  Its
    // waiter sends ImageOutputComplete when the file is complete and gives the slot back.
    std::thread image_waiter;
    golhip_image *image_begun = nullptr;  // begun, its waiter not yet started
    auto image_join = [&] {
        if (image_waiter.joinable()) image_waiter.join();
    };
    auto stop_helpers = [&] {
        {
            std::lock_guard<std::mutex> lk(tick_mu);
            finished = true;
        }
        tick_cv.notify_all();
        if (ticker.joinable()) ticker.join();
        if (keys.joinable()) keys.join();
        image_join();
        if (helper_err) std::rethrow_exception(helper_err);
    };

    try {
        // The turn loop in batches (distributor.go:93-173): each engine call
        // runs up to `batch` turns; with cell events it is the fused flip
        // stream (golhip_flip_stream: every turn's CellFlipped list, written
        // by the device straight into a page-locked buffer as cell indices),
        // otherwise fused step launches.  `mu` is held only for the call, so
        // the ticker, s/q snapshots and p (which takes `mu`, as the
        // reference's pause does) act between batches, at a turn boundary.
        // with a view stream a batch ends on a frame and fills at most half the ring
        const bool view_stream = view_on && !opt.cell_events;
        const int64_t batch = !view_stream ? batch_turns
                                           : std::max<int64_t>(1, std::min(batch_turns / opt.view_every, ring->per_half)) *
                                                 opt.view_every;
        FlipBuffer fb;
        if (opt.cell_events) fb.grow((uint64_t)std::min<int64_t>(W * H * std::min<int64_t>(batch, 4), 64ll << 20));
        std::vector<uint64_t> counts((size_t)batch);
        constexpr uint64_t kFlipChunk = 4096;
        std::vector<Event> flip_evs;
        int64_t t = T0;
        while (t < p.Turns && !quit.load()) {
            int64_t want = std::min<int64_t>(batch, p.Turns - t);
            // an engine call ends on every checkpoint turn
            if (opt.checkpoint_every > 0) want = std::min(want, opt.checkpoint_every - t % opt.checkpoint_every);
            if (opt.image_every > 0) want = std::min(want, opt.image_every - t % opt.image_every);  // and on every image turn
            if (view_on && !view_stream) want = std::min(want, opt.view_every - t % opt.view_every);  // end on a frame turn
            // a view stream's frames stay on the multiples of view_every: a call begun off one (behind
            // a checkpoint turn or a resume; never otherwise) steps to the next and renders there
            const bool streamed = view_stream && t % opt.view_every == 0;
            if (view_stream && !streamed) want = std::min(want, opt.view_every - t % opt.view_every);
            int64_t done = want;
            uint64_t n = 0;
            int view_half = 0;
            bool ckpt_due = false, image_due = false;
            {
                std::lock_guard<std::mutex> g(mu);
                if (quit.load()) break;  // `q` took its snapshot while this thread waited for `mu`
                if (streamed) {
                    // frame i of the batch shows turn t + (i + 1) * every
                    uint64_t nf = 0;
                    view_half = ring->half;
                    check(golhip_group_view_stream(board.hs.data(), (int32_t)board.hs.size(), want, opt.view_every,
                                                   &opt.view, ring->slot(view_half, 0), (uint64_t)ring->per_half, &nf,
                                                   &done));
                    ring->half ^= 1;
                } else if (opt.cell_events) {
                    int rc = board.flip_stream(want, fb, counts.data(), &done, &n);
                    if (rc == GOLHIP_ERANGE) {  // one turn needs more than the buffer: grow, nothing advanced
                        fb.grow(n);
                        rc = board.flip_stream(want, fb, counts.data(), &done, &n);
                    }
                    check(rc);
                } else {
                    board.step(want);
                }
                t += done;
                turn = t;
                if (view_on && !streamed && t % opt.view_every == 0) view_now();  // ahead of the batch's events
                ckpt_due = opt.checkpoint_every > 0 && done > 0 && t % opt.checkpoint_every == 0;
                image_due = opt.image_every > 0 && done > 0 && t % opt.image_every == 0;
            }
            if (image_due) {
                // as the checkpoint below: the previous image's writer is joined off `mu`, the enqueue is on it
                // (and an `s` / `q` image in flight finishes first: the slot)
                image_join();
                image_slot.acquire();
                try {
                    board.drain_wait();
                    std::lock_guard<std::mutex> g(mu);
                    image_begun = image_begin(t);
                } catch (...) {
                    image_slot.release();
                    throw;
                }
            }
            if (ckpt_due) {
                // the previous checkpoint's writer (fsync, rename) is joined off `mu`, so the ticker and the
                // keys are not held up by the file system; only the enqueue is a turn-boundary action
                board.ckpt_wait();
                board.drain_wait();  // (an image begun on this turn or by a key: its shadow drains off `mu` too)
                std::lock_guard<std::mutex> g(mu);
                board.ckpt_begin(opt.checkpoint_path, t);
            }
            // let a queued ticker / key handler take `mu` before the next batch
            while (waiters.load() > 0) std::this_thread::sleep_for(std::chrono::microseconds(20));
            const int64_t t0 = t - done;
            uint64_t off = 0;
            for (int64_t i = 0; i < done; ++i) {
                const int64_t completed = t0 + i + 1;  // quirks: the reference's 0-based turn (:113, :171, :216)
                if (opt.cell_events) {
                    // initializeAliveCells (:212-220): the turn's list, in order, sent in
                    // chunks (Chan::send_batch: one lock a chunk on a buffered channel)
                    const uint64_t n = counts[(size_t)i];
                    for (uint64_t e0 = off; e0 < off + n && events; e0 += kFlipChunk) {
                        const uint64_t m = std::min<uint64_t>(kFlipChunk, off + n - e0);
                        flip_evs.resize(m);
                        for (uint64_t j = 0; j < m; ++j) {
                            const uint64_t idx = fb.p[e0 + j];
                            Event &ev = flip_evs[j];
                            ev.kind = EventKind::CellFlipped;
                            ev.CompletedTurns = quirks ? completed - 1 : completed;
                            ev.Cell.X = quirks ? (int64_t)(idx / W) : (int64_t)(idx % W);
                            ev.Cell.Y = quirks ? (int64_t)(idx % W) : (int64_t)(idx / W);
                        }
                        events->send_batch(flip_evs.data(), m);
                    }
                    off += n;
                }
                if (streamed && (i + 1) % opt.view_every == 0)  // (t0 is a multiple of every)
                    opt.view_sink->publish(ring->slot(view_half, (i + 1) / opt.view_every - 1), ring->frame_bytes,
                                           completed);
                if (opt.turn_events) {
                    Event ev;
                    ev.kind = EventKind::TurnComplete;
                    ev.CompletedTurns = quirks ? completed - 1 : completed;
                    send(ev);
                }
            }
            if (image_begun) {
                // behind the turn's own events: ImageOutputComplete{t} follows TurnComplete{t}
                golhip_image *im = image_begun;
                image_begun = nullptr;
                const int64_t at = t;
                image_waiter = std::thread(guarded([&, im, at] {
                    SlotRelease slot{&image_slot};
                    image_finish(im, at);
                }));
            }
        }
        stop_helpers();
        if (view_on && opt.view_sink->turn() != turn.load()) view_now();  // turns after the last frame
        if (quit.load()) {
            // `q` (:244-261): snapshot already written; the reference os.Exit(0)s
            // without FinalTurnComplete.  The mirror ends the run instead; with
            // checkpointing on it first leaves the state a new controller takes over.
            if (ckpt_on) {
                if (board.ckpt_turn != turn.load()) board.ckpt_begin(opt.checkpoint_path, turn.load());
                board.ckpt_wait();
            }
            Event e;
            e.kind = EventKind::StateChange;
            e.CompletedTurns = turn.load();
            e.NewState = State::Quitting;
            send(e);
            if (events) events->close();
            return;
        }
        board.ckpt_wait();  // the last periodic checkpoint is on disk before FinalTurnComplete
        // distributor.go:180-206
        std::vector<util::Cell> alive = board.cells(golhip_alive_cells, false);
        write_rle(p.Turns);
        if (stream) {
            image_finish(image_begin(p.Turns), p.Turns);  // the run never holds W * H bytes
        } else {
            const std::string fname = write_snapshot(p.Turns, false);
            Event io;
            io.kind = EventKind::ImageOutputComplete;
            io.CompletedTurns = p.Turns;
            io.Filename = fname;
            send(io);
        }
        Event fin;
        fin.kind = EventKind::FinalTurnComplete;
        fin.CompletedTurns = p.Turns;
        fin.Alive = std::move(alive);
        send(fin);
        Event q;
        q.kind = EventKind::StateChange;
        q.CompletedTurns = p.Turns;
        q.NewState = State::Quitting;
        send(q);
        if (events) events->close();
    } catch (...) {
        if (image_begun) {
            golhip_image_wait(image_begun, nullptr);
            image_slot.release();
        }
        stop_helpers();
        if (events) events->close();
        throw;
    }
}

}  // namespace gol

// ---------------------------------------------------------------------------
// C-ABI of the host mirror (include/golrun.h): lets non-C++ callers (the
// Python parity tests) drive gol::Run the way gol_test.go drives gol.Run.
// ---------------------------------------------------------------------------
struct golrun {
    gol::Chan<gol::Event> events;
    gol::Chan<char32_t> keys;
    bool use_keys;
    std::thread th;
    std::string err;
    std::atomic<bool> done{false};
    gol::Event current;
    bool has_view = false;
    gol::ViewSink view;
    golrun(size_t cap, bool k) : events(cap), keys(16), use_keys(k) {}
};

namespace {
thread_local std::string g_run_err;
int run_fail(const std::string &m) {
    g_run_err = m;
    return GOLHIP_EINVAL;
}
}  // namespace

extern "C" {

const char *golrun_last_error(void) { return g_run_err.c_str(); }

int golrun_start(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root, int32_t device,
                 uint32_t flags, int32_t events_cap, int32_t ticker_ms, golrun_t *out) {
    return golrun_start_view(turns, threads, width, height, root, device, flags, events_cap, ticker_ms, nullptr, 1, out);
}

int golrun_view_frame(golrun_t r, void *out, uint64_t cap_bytes, int64_t *turn) {
    if (!r || !out) return run_fail("bad arguments");
    if (!r->has_view) return run_fail("the run has no view (golrun_start_view)");
    uint64_t bytes = 0;
    switch (r->view.fetch(out, cap_bytes, turn, &bytes)) {
    case 0: return GOLHIP_OK;
    case 1: return run_fail("no frame published yet");
    default:
        g_run_err = "buffer holds " + std::to_string(cap_bytes) + " bytes, the frame needs " + std::to_string(bytes);
        return GOLHIP_ERANGE;
    }
}

int golrun_start_view(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root,
                      int32_t device, uint32_t flags, int32_t events_cap, int32_t ticker_ms,
                      const golhip_view_t *view, int32_t every, golrun_t *out) {
    golrun_opts_t opts;
    memset(&opts, 0, sizeof opts);
    opts.view = view;
    opts.view_every = every;
    return golrun_start_opts(turns, threads, width, height, root, device, flags, events_cap, ticker_ms, &opts, out);
}

int golrun_start_opts(int64_t turns, int64_t threads, int64_t width, int64_t height, const char *root,
                      int32_t device, uint32_t flags, int32_t events_cap, int32_t ticker_ms,
                      const golrun_opts_t *opts, golrun_t *out) {
    if (!out || !root || events_cap < 0) return run_fail("bad arguments");
    golrun_opts_t none;
    memset(&none, 0, sizeof none);
    none.view_every = 1;
    if (!opts) opts = &none;
    const golhip_view_t *view = opts->view;
    const int32_t every = opts->view_every;
    if (view && (view->scale < 1 || every < 1)) return run_fail("view scale and every must be >= 1");
    if (opts->checkpoint_every < 0 || (opts->checkpoint_every > 0 && !(opts->checkpoint_path && *opts->checkpoint_path)))
        return run_fail("checkpoint_every must be >= 0 and needs checkpoint_path");
    gol::Params p;
    p.Turns = turns;
    p.Threads = threads;
    p.ImageWidth = width;
    p.ImageHeight = height;
    gol::RunOptions o;
    o.root = root;
    o.device = device;
    o.ref_quirks = (flags & GOLRUN_FLAG_REF_QUIRKS) != 0;
    o.cell_events = (flags & GOLRUN_FLAG_NO_CELL_EVENTS) == 0;
    o.turn_events = (flags & GOLRUN_FLAG_NO_TURN_EVENTS) == 0;
    if (ticker_ms > 0) o.ticker_seconds = ticker_ms / 1000.0;
    if (opts->checkpoint_path) o.checkpoint_path = opts->checkpoint_path;
    o.checkpoint_every = opts->checkpoint_every;
    if (opts->resume_path) o.resume_path = opts->resume_path;
    if (opts->reserved[1] != 0) o.stream_images = 1;
    o.image_every = opts->reserved[0];
    o.blank = opts->reserved[3] != 0;
    if (opts->reserved0 != 0) {  // the rule: 0x40000 | survive << 9 | birth
        if ((opts->reserved0 & ~0x7FFFF) != 0 || !(opts->reserved0 & 0x40000)) return run_fail("bad rule word in reserved0");
        o.rule.birth = (uint32_t)opts->reserved0 & 0x1FF;
        o.rule.survive = ((uint32_t)opts->reserved0 >> 9) & 0x1FF;
    }
    if (opts->reserved[2]) {  // one "path@x,y[,op]" a line
        std::stringstream lines(reinterpret_cast<const char *>((uintptr_t)opts->reserved[2]));
        try {
            for (std::string line; std::getline(lines, line);)
                if (!line.empty()) o.patterns.push_back(gol::ParsePattern(line));
        } catch (const std::exception &e) {
            return run_fail(e.what());
        }
    }
    golrun *r = new golrun((size_t)events_cap, (flags & GOLRUN_FLAG_KEYS) != 0);
    if (flags & GOLRUN_FLAG_VIEW_STRIPS) o.view_strips = 1;
    if (flags & GOLRUN_FLAG_SAVE_RLE) o.save_rle = 1;
    if (flags & GOLRUN_FLAG_RULE_FLIPS) o.rule_flips = 1;
    if (flags & GOLRUN_FLAG_PLANE) o.plane = 1;
    if (view) {
        r->has_view = true;
        o.view = *view;
        o.view_every = every;
        o.view_sink = &r->view;
    }
    r->th = std::thread([r, p, o] {
        try {
            gol::Run(p, &r->events, r->use_keys ? &r->keys : nullptr, o);
        } catch (const std::exception &e) {
            r->err = e.what();
            r->events.close();
        }
        r->done = true;
    });
    *out = r;
    return GOLHIP_OK;
}

int golrun_next_event(golrun_t r, golrun_event_t *ev, int32_t timeout_ms) {
    if (!r || !ev) return run_fail("bad arguments");
    const auto t_end = std::chrono::steady_clock::now() + std::chrono::milliseconds(timeout_ms < 0 ? 0 : timeout_ms);
    for (;;) {
        int got = r->events.try_recv(r->current);
        if (got == 1) break;
        if (got < 0) return 0;  // closed and drained: the `range events` loop ends
        if (timeout_ms >= 0 && std::chrono::steady_clock::now() >= t_end) return 2;
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
    const gol::Event &e = r->current;
    memset(ev, 0, sizeof *ev);
    ev->kind = (int32_t)e.kind;
    ev->completed_turns = e.CompletedTurns;
    ev->cells_count = e.CellsCount;
    ev->new_state = (int32_t)e.NewState;
    ev->cell_x = e.Cell.X;
    ev->cell_y = e.Cell.Y;
    ev->alive_len = (int64_t)e.Alive.size();
    std::snprintf(ev->filename, sizeof ev->filename, "%s", e.Filename.c_str());
    std::snprintf(ev->text, sizeof ev->text, "%s", e.String().c_str());
    return 1;
}

int golrun_event_string(const golrun_event_t *ev, char *out, uint64_t cap) {
    if (!ev || !out || cap == 0) return run_fail("bad arguments");
    gol::Event e;
    e.kind = (gol::EventKind)ev->kind;
    e.CompletedTurns = ev->completed_turns;
    e.CellsCount = ev->cells_count;
    e.NewState = (gol::State)ev->new_state;
    e.Filename = std::string(ev->filename, strnlen(ev->filename, sizeof ev->filename));
    std::snprintf(out, cap, "%s", e.String().c_str());
    return GOLHIP_OK;
}

int golrun_event_cells(golrun_t r, int64_t *xy, uint64_t cap) {
    if (!r) return run_fail("bad arguments");
    const auto &a = r->current.Alive;
    if (cap < a.size() || (!xy && !a.empty())) return run_fail("buffer too small");
    for (size_t i = 0; i < a.size(); ++i) {
        xy[2 * i] = a[i].X;
        xy[2 * i + 1] = a[i].Y;
    }
    return GOLHIP_OK;
}

int golrun_drain(golrun_t r, golrun_drain_stats_t *st, uint64_t *flips, uint64_t *digests, int64_t turns_cap,
                 int64_t width) {
    if (!r || !st || turns_cap < 0 || ((flips || digests) && width <= 0)) return run_fail("bad arguments");
    memset(st, 0, sizeof *st);
    for (int64_t t = 0; t < turns_cap; ++t) {
        if (flips) flips[t] = 0;
        if (digests) digests[t] = 0;
    }
    auto mix = [](uint64_t x) {
        uint64_t z = x + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    };
    std::vector<gol::Event> batch;
    batch.reserve(1024);
    while (r->events.recv_batch(batch, 1024)) {  // main.go:59-66, until close (every event, in order)
        for (const gol::Event &e : batch) {
            const int k = (int)e.kind;
            if (k >= 0 && k < 6) st->count[k]++;
            if (e.kind == gol::EventKind::TurnComplete) st->last_turn = e.CompletedTurns;
            if (e.kind == gol::EventKind::FinalTurnComplete) st->final_alive = (int64_t)e.Alive.size();
            if (e.kind != gol::EventKind::CellFlipped || e.CompletedTurns < 1 || e.CompletedTurns > turns_cap)
                continue;
            const int64_t t = e.CompletedTurns - 1;
            const uint64_t i = flips ? ++flips[t] : 0;
            if (digests) digests[t] += mix(i) * ((uint64_t)e.Cell.Y * (uint64_t)width + (uint64_t)e.Cell.X + 1);
        }
    }
    return GOLHIP_OK;
}

int golrun_send_key(golrun_t r, uint32_t key) {
    if (!r || !r->use_keys) return run_fail("run has no key channel");
    return r->keys.send((char32_t)key) ? GOLHIP_OK : run_fail("key channel closed");
}

int golrun_wait(golrun_t r, char *err, uint64_t err_cap) {
    if (!r) return run_fail("bad arguments");
    // drain whatever the caller left unread so the run can finish
    gol::Event tmp;
    while (!r->done.load()) {
        if (r->events.try_recv(tmp) == 0) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    if (r->th.joinable()) r->th.join();
    if (err && err_cap) std::snprintf(err, err_cap, "%s", r->err.c_str());
    return r->err.empty() ? GOLHIP_OK : GOLHIP_EINVAL;
}

int golrun_destroy(golrun_t r) {
    if (!r) return GOLHIP_OK;
    golrun_wait(r, nullptr, 0);
    delete r;
    return GOLHIP_OK;
}

}  // extern "C"
