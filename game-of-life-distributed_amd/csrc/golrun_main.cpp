// golrun — the reference's command line (main.go:13-66) over the C++ mirror
// of gol.Run (gol_host.h) and libgolhip.so.
//
//   golrun [-t threads] [-w width] [-h height] [-turns n] [-noVis] [-root dir] [-device n]
//          [-viewScale n] [-viewEvery n] [-viewDir dir] [-viewStrips]
//          [-checkpoint path] [-checkpointEvery n] [-resume path]
//          [-streamImages] [-imageEvery n] [-blank] [-pattern path@x,y[,op]]... [-saveRle]
//          [-rule B36/S23[:P<w>,<h>]] [-ruleFlips] [-plane]
//
// Same flags, defaults and output as main.go: "Threads: / Width: / Height:"
// lines, then gol.Run on images/<w>x<h>.pgm with an events channel of
// capacity 1000 and a keyPresses channel of capacity 10.  There is no SDL
// window in this build (sdl/ is out of scope): without -noVis
// the run is headless too, and single-character lines on stdin (s, q, p, k)
// are forwarded as key presses, the keys the SDL loop forwards (sdl/loop.go).
// -viewScale n (0 = off, the default) renders the whole board on the device,
// one GRAY8 pixel per n x n cells (width / n x height / n pixels), after every
// -viewEvery-th turn (default 1) and writes every frame as
// <viewDir>/view_<W>x<H>x<turn>.pgm (P5; -viewDir defaults to <root>/out/view):
// the pixels a window would show (gol_host.h RunOptions::view).  On row strips
// (GOL_STRIPS / GOL_NGPU) a view needs -viewStrips (or GOL_VIEW_STRIPS=1): the
// frames are then rendered across the strips, the same pixels.
// -checkpoint <path> with -checkpointEvery <n> (turns; 0 = off, the default)
// writes a checkpoint of the board to <path> at every turn that is a multiple
// of n, behind the following turns, and on `q` one of the turn the run stops
// at; -resume <path> starts from such a file, at its turn, instead of
// images/<w>x<h>.pgm (gol_host.h RunOptions::checkpoint_path, resume_path).
// -streamImages (or GOL_STREAM_IMAGES=1) reads images/<w>x<h>.pgm chunk by
// chunk and writes the out/ images behind the following turns, never holding
// a whole raster on the host; with it, -imageEvery <n> writes
// out/<w>x<h>x<turn>.pgm at every turn that is a multiple of n
// (gol_host.h RunOptions::stream_images, image_every).
// -blank starts from an empty board instead of images/<w>x<h>.pgm; -pattern
// path@x,y[,op] (repeatable; op one of copy|or|xor|clear, default or) stamps
// a pattern file (RLE or PGM) with its top-left corner at the torus cell
// (x, y), in the order given, before the first event (gol_host.h
// RunOptions::blank, patterns).  A bad spec or an unreadable file ends the run
// with the parser's message, before any event.
// -saveRle writes out/<w>x<h>x<turn>.rle, the alive box of the board, beside
// the final image and the images of s and q (gol_host.h RunOptions::save_rle);
// an empty board writes none.
// -rule B36/S23 runs another Life-like rule than Conway's (golhip_rule_parse's
// spellings; gol_host.h RunOptions::rule); a rule that does not parse ends the
// run with the parser's message, before any event.  -ruleFlips (or
// GOL_RULE_FLIPS=1) takes such a run's CellFlipped batches from the fused turn
// + list kernel (gol_host.h RunOptions::rule_flips); the events are the same.
// -plane (or GOL_PLANE=1) runs the board as a bounded plane: every cell outside
// it is dead for ever (gol_host.h RunOptions::plane).  -rule takes Golly's
// bounded-grid suffix too: "B3/S23:P512,512" is -plane and "B3/S23:T512,512" the
// torus, where the bounds equal -w and -h; any other bounds end the run with a
// message, before any event (a board is as large as its image).  Of several
// -rule flags the last one counts, suffix included (a later -rule without one
// is the environment's topology again); -plane or -plane=false wins over a suffix.
// The headless drain loop ends at FinalTurnComplete (main.go:59-66) or when
// the events channel closes.
#include <sys/stat.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <thread>

#include "gol_host.h"

namespace {

[[noreturn]] void usage(const char *msg) {
    std::fprintf(stderr, "golrun: %s\nusage: golrun [-t threads] [-w width] [-h height] [-turns n] [-noVis] "
                         "[-root dir] [-device n] [-viewScale n] [-viewEvery n] [-viewDir dir] [-viewStrips] "
                         "[-checkpoint path] [-checkpointEvery n] [-resume path] [-streamImages] [-imageEvery n] [-blank] "
                         "[-pattern path@x,y[,op]]... [-rule B36/S23[:P<w>,<h>]] [-ruleFlips] [-plane] [-saveRle]\n", msg);
    std::exit(2);
}

long long parse_int(const std::string &s, const char *flag) {
    char *end = nullptr;
    const long long v = std::strtoll(s.c_str(), &end, 10);
    if (s.empty() || *end) usage((std::string("invalid value \"") + s + "\" for flag -" + flag).c_str());
    return v;
}

}  // namespace

int main(int argc, char **argv) {
    gol::Params params;
    params.Threads = 8;
    params.ImageWidth = 512;
    params.ImageHeight = 512;
    long long turns = 10000000000LL;  // main.go:37-41
    bool no_vis = false;
    gol::RunOptions opt;
    long long view_scale = 0, view_every = 1;
    std::string view_dir;
    std::string rule_text;              // -rule's text where it names bounds ...
    int32_t rule_bw = 0, rule_bh = 0;   // ... and the bounds, held against -w / -h once every flag is read
    int rule_plane = -1, flag_plane = -1;  // the topology the last -rule's suffix names (-1: none) and -plane's
    for (int i = 1; i < argc; ++i) {
        std::string a = argv[i];
        if (a.rfind("--", 0) == 0) a = a.substr(1);  // Go's flag package accepts -flag and --flag
        std::string key = a, val;
        const size_t eq = a.find('=');
        if (eq != std::string::npos) {
            key = a.substr(0, eq);
            val = a.substr(eq + 1);
        }
        auto value = [&]() -> std::string {
            if (eq != std::string::npos) return val;
            if (i + 1 >= argc) usage(("flag needs an argument: " + key).c_str());
            return argv[++i];
        };
        if (key == "-t") {
            params.Threads = parse_int(value(), "t");
        } else if (key == "-w") {
            params.ImageWidth = parse_int(value(), "w");
        } else if (key == "-h") {
            params.ImageHeight = parse_int(value(), "h");
        } else if (key == "-turns") {
            turns = parse_int(value(), "turns");
        } else if (key == "-noVis") {
            no_vis = eq == std::string::npos || val == "true" || val == "1";
        } else if (key == "-root") {
            opt.root = value();
        } else if (key == "-device") {
            opt.device = (int)parse_int(value(), "device");
        } else if (key == "-viewScale") {
            view_scale = parse_int(value(), "viewScale");
        } else if (key == "-viewEvery") {
            view_every = parse_int(value(), "viewEvery");
        } else if (key == "-viewDir") {
            view_dir = value();
        } else if (key == "-viewStrips") {
            opt.view_strips = (eq == std::string::npos || val == "true" || val == "1") ? 1 : 0;
        } else if (key == "-checkpoint") {
            opt.checkpoint_path = value();
        } else if (key == "-checkpointEvery") {
            opt.checkpoint_every = parse_int(value(), "checkpointEvery");
        } else if (key == "-resume") {
            opt.resume_path = value();
        } else if (key == "-streamImages") {
            opt.stream_images = (eq == std::string::npos || val == "true" || val == "1") ? 1 : 0;
        } else if (key == "-imageEvery") {
            opt.image_every = parse_int(value(), "imageEvery");
        } else if (key == "-blank") {
            opt.blank = eq == std::string::npos || val == "true" || val == "1";
        } else if (key == "-saveRle") {
            opt.save_rle = (eq == std::string::npos || val == "true" || val == "1") ? 1 : 0;
        } else if (key == "-ruleFlips") {
            opt.rule_flips = (eq == std::string::npos || val == "true" || val == "1") ? 1 : 0;
        } else if (key == "-rule") {
            const std::string text = value();
            int32_t topology = GOLHIP_TOPOLOGY_TORUS;
            if (golhip_rule_parse_ex(text.c_str(), &opt.rule.birth, &opt.rule.survive, &topology, &rule_bw, &rule_bh) !=
                GOLHIP_OK) {
                std::fprintf(stderr, "golrun: %s\n", golhip_last_error());
                return 1;
            }
            rule_text = text;
            // the last -rule alone decides what -rule says of the topology: a text without a suffix says nothing
            rule_plane = rule_bw > 0 ? (topology == GOLHIP_TOPOLOGY_PLANE ? 1 : 0) : -1;
        } else if (key == "-plane") {
            flag_plane = (eq == std::string::npos || val == "true" || val == "1") ? 1 : 0;
        } else if (key == "-pattern") {
            try {
                opt.patterns.push_back(gol::ParsePattern(value()));
            } catch (const std::exception &e) {
                std::fprintf(stderr, "golrun: %s\n", e.what());
                return 1;
            }
        } else {
            usage(("flag provided but not defined: " + key).c_str());
        }
    }
    if (opt.checkpoint_every < 0 || (opt.checkpoint_every > 0 && opt.checkpoint_path.empty()))
        usage("-checkpointEvery must be >= 0 and needs -checkpoint <path>");
    if (rule_bw > 0 && (rule_bw != params.ImageWidth || rule_bh != params.ImageHeight)) {
        std::fprintf(stderr, "golrun: rule \"%s\": the bounds %d x %d are not the board's %lld x %lld (-w, -h)\n",
                     rule_text.c_str(), rule_bw, rule_bh, (long long)params.ImageWidth, (long long)params.ImageHeight);
        return 1;
    }
    opt.plane = flag_plane >= 0 ? flag_plane : rule_plane;  // -plane[=false] wins over a suffix; neither: GOL_PLANE
    params.Turns = turns;  // a Go int (64-bit): the reference's 10^10 default passes through

    std::printf("Threads: %lld\nWidth: %lld\nHeight: %lld\n", (long long)params.Threads, (long long)params.ImageWidth,
                (long long)params.ImageHeight);
    std::fflush(stdout);
    if (!no_vis) std::fprintf(stderr, "golrun: no SDL window in this build; running headless (keys s/q/p/k on stdin)\n");

    // live view: every published frame of the whole board goes to a PGM file
    gol::ViewSink sink;
    std::string view_error;
    if (view_scale != 0) {
        if (view_scale < 1 || view_scale > GOLHIP_VIEW_MAX_SCALE || view_every < 1 ||
            view_scale > params.ImageWidth || view_scale > params.ImageHeight)
            usage("-viewScale must be in [1, 1024] and at most the board's sides, -viewEvery >= 1");
        if (view_dir.empty()) view_dir = opt.root + "/out/view";
        opt.view = golhip_view_t{0, 0, (int32_t)view_scale, (int32_t)(params.ImageWidth / view_scale),
                                 (int32_t)(params.ImageHeight / view_scale), GOLHIP_VIEW_GRAY8};
        opt.view_every = view_every;
        opt.view_sink = &sink;
        const std::string stem = view_dir + "/view_" + std::to_string(params.ImageWidth) + "x" +
                                 std::to_string(params.ImageHeight) + "x";
        const std::string out_dir = opt.root + "/out";
        const gol::RunOptions &o = opt;
        sink.on_publish = [stem, out_dir, view_dir, &o, &view_error](const void *frame, uint64_t, int64_t turn) {
            try {
                mkdir(out_dir.c_str(), 0777);
                mkdir(view_dir.c_str(), 0777);
                gol::WritePgm(stem + std::to_string(turn) + ".pgm", o.view.out_w, o.view.out_h,
                              static_cast<const uint8_t *>(frame));
            } catch (const std::exception &e) {
                if (view_error.empty()) view_error = e.what();
            }
        };
    }

    gol::Chan<char32_t> keys(10);
    gol::Chan<gol::Event> events(1000);
    std::string error;
    std::thread engine([&] {
        try {
            gol::Run(params, &events, &keys, opt);
        } catch (const std::exception &e) {
            error = e.what();
            events.close();
        }
    });
    if (!no_vis) {
        std::thread([&keys] {  // detached: blocks on stdin until the process ends
            std::string line;
            while (std::getline(std::cin, line))
                if (line.size() == 1 && std::strchr("sqpk", line[0])) keys.send((char32_t)line[0]);
        }).detach();
    }
    gol::Event ev;
    while (events.recv(ev)) {  // main.go:59-66
        if (ev.kind == gol::EventKind::FinalTurnComplete) break;
    }
    while (events.recv(ev)) {  // let Run finish (StateChange Quitting, close)
    }
    engine.join();
    if (error.empty()) error = view_error;
    if (!error.empty()) {
        std::fprintf(stderr, "golrun: %s\n", error.c_str());
        return 1;
    }
    return 0;
}
