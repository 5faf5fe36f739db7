// tests/debug/sequence_probe.cpp -- the submission sequencer (csrc/submit_sequence.cpp) on its own: no HIP, no device.
// tests/test_submit_sequence.py compiles this file with submit_sequence.cpp under -fsanitize=address,undefined and runs it as a child.
//
//   sequence_probe SCRIPT        one JSON line per event of the file SCRIPT (none for `new` and `fail`); addresses are decimal integers:
//       new                                  a fresh sequencer, calls counted from 0 again
//       apply EYE TEX W H PITCH FMT DST W H PITCH FMT PAIRMODE STAGES ONLYONEEYE
//                                            one Apply behind its checks: TEX is the texture (the address of `in`), DST the resolved destination
//       batch                                a batch call arrives: a recorded submission goes first
//       size KEEP                            the input size changes: a recorded submission goes first, then the implicit reset, which keeps the
//                                            learned order (KEEP = 1: the flushed eye was handed a ctx-owned image) or forgets it (0)
//       reset                                an explicit reset
//       fail flush | fail main               the next event's flush / launch fails
//       pairable A W H PITCH FMT (x4)        the predicate alone, images in the order first in, first out, second in, second out
//   An apply line reports the steps decided, the launches that succeeded as lists of call numbers ([k]: call k alone, [j, k]: the batch of
//   two), the address handed back and the sequencer's state afterwards.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include "../../openvr_fsr_amd/csrc/submit_sequence.h"

using namespace ovrfsr;

static bool read_image(std::istream &is, ovrfsr_image *img)
{
    unsigned long long a = 0;
    if (!(is >> a >> img->width >> img->height >> img->pitch_bytes >> img->format)) return false;
    img->data = reinterpret_cast<void *>(static_cast<uintptr_t>(a));
    return true;
}

static unsigned long long addr(const ovrfsr_image &img) { return static_cast<unsigned long long>(reinterpret_cast<uintptr_t>(img.data)); }

static void print_state(const SubmitSequencer &q)
{
    const SubmitSequencer::State &s = q.state();
    std::printf("\"state\": {\"pending\": %d, \"pending_eye\": %d, \"pending_in\": %llu, \"pending_out\": %llu, \"first_eye\": %d, \"defer\": %d, "
                "\"last_eye\": %d, \"recorded\": %d, \"last_texture\": %llu, \"eye_count\": %d, \"output\": %llu, \"pair_pending\": %d}}\n",
                (int)s.havePending, s.pendingEye, s.havePending ? addr(s.pendingIn) : 0ull, s.havePending ? addr(s.pendingOut) : 0ull, s.pairFirstEye,
                (int)s.pairDefer, s.lastEye, (int)s.lastApplyRecorded, (unsigned long long)s.lastSubmittedTexture, s.eyeCount, addr(s.outputTexture),
                (int)q.PairPending());
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: sequence_probe SCRIPT\n"); return 2; }
    std::ifstream f(argv[1]);
    if (!f) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    SubmitSequencer q;
    int call = 0, recordedCall = -1;
    bool failFlush = false, failMain = false;
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string ev;
        if (!(is >> ev)) continue;
        if (ev == "new") {
            q = SubmitSequencer();
            call = 0; recordedCall = -1; failFlush = failMain = false;
        } else if (ev == "fail") {
            std::string what;
            is >> what;
            (what == "flush" ? failFlush : failMain) = true;
        } else if (ev == "reset") {
            q.Reset(true);
            std::printf("{\"ev\": \"reset\", \"steps\": [], \"launches\": [], \"failed\": null, ");
            print_state(q);
        } else if (ev == "batch" || ev == "size") {
            Submission s;
            const bool flush = q.TakeRecorded(&s);
            const bool failed = flush && failFlush;
            std::printf("{\"ev\": \"%s\", \"steps\": [%s], \"launches\": [", ev.c_str(), flush ? "\"flush\"" : "");
            if (flush && !failed) std::printf("[%d]", recordedCall);
            std::printf("], \"failed\": %s, ", failed ? "\"flush\"" : "null");
            int keep = 0;
            is >> keep;
            if (!failed && ev == "size") q.Reset(!(flush && keep));
            print_state(q);
            failFlush = failMain = false;
        } else if (ev == "apply") {
            int eye = 0, pairMode = 0, stages = 0, onlyOneEye = 0;
            ovrfsr_image in = {}, dst = {};
            if (!(is >> eye) || !read_image(is, &in) || !read_image(is, &dst) || !(is >> pairMode >> stages >> onlyOneEye)) {
                std::fprintf(stderr, "bad apply line: %s\n", line.c_str());
                return 2;
            }
            const SubmitSequencer::Steps st = q.Begin(eye, in, dst, pairMode != 0, stages != 0, onlyOneEye != 0);
            static const char *const names[] = {"forward", "reuse", "record", "pair", "single"};
            std::string launches;
            const char *failed = "null";
            bool ok = true;
            if (st.flush) {
                if (failFlush) { ok = false; failed = "\"flush\""; }
                else { q.FlushDone(st); launches += "[" + std::to_string(recordedCall) + "]"; }
            }
            const bool launchesSomething = st.images != 0;
            unsigned long long returned = 0;
            if (ok && launchesSomething && failMain) { ok = false; failed = "\"main\""; }
            if (ok) {
                if (launchesSomething) {
                    if (!launches.empty()) launches += ", ";
                    launches += st.action == SubmitSequencer::Action::LaunchPair ? "[" + std::to_string(recordedCall) + ", " + std::to_string(call) + "]"
                                                                                 : "[" + std::to_string(call) + "]";
                }
                returned = addr(q.Finish(st));
                if (st.action == SubmitSequencer::Action::Record) recordedCall = call;
            }
            std::printf("{\"ev\": \"apply\", \"call\": %d, \"steps\": [%s\"%s\"], \"launches\": [%s], \"failed\": %s, \"returned\": %llu, ", call,
                        st.flush ? "\"flush\", " : "", names[(int)st.action], launches.c_str(), failed, returned);
            if (st.action == SubmitSequencer::Action::LaunchPair)
                std::printf("\"pair_eye\": %d, \"in_stride\": %llu, \"out_stride\": %llu, ", st.launch.eye, (unsigned long long)st.inStride, (unsigned long long)st.outStride);
            if (st.action == SubmitSequencer::Action::LaunchSingle) std::printf("\"single_eye\": %d, ", st.launch.eye);
            print_state(q);
            ++call;
            failFlush = failMain = false;
        } else if (ev == "pairable") {
            ovrfsr_image im[4] = {};
            for (ovrfsr_image &i : im)
                if (!read_image(is, &i)) { std::fprintf(stderr, "bad pairable line: %s\n", line.c_str()); return 2; }
            size_t inStride = 0, outStride = 0;
            const bool p = pairable(im[0], im[1], im[2], im[3], &inStride, &outStride);
            std::printf("{\"pairable\": %d, \"in_stride\": %llu, \"out_stride\": %llu}\n", (int)p, (unsigned long long)inStride, (unsigned long long)outStride);
        } else {
            std::fprintf(stderr, "unknown event: %s\n", line.c_str());
            return 2;
        }
    }
    return 0;
}
