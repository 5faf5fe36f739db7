// submit_sequence.h -- what one ovrfsr_apply does with its submission, decided on the host before anything is launched: handed back, answered
// with the previous output, recorded as a frame's first eye (cfg.pair_submit), launched alone, or launched as a batch of two with the recorded
// one.  SubmitSequencer is pure: no HIP call, no device; image addresses are integers to it.  PostProcessor::Apply (postprocessor.cpp) asks,
// launches what it is told, and reports back; tests/debug/sequence_probe.cpp runs the sequencer alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/openvr_fsr_amd.h"

namespace ovrfsr {

// the kernels read neighbours of what other workgroups write: do the byte ranges of n input and n output images overlap?
bool ranges_overlap(const ovrfsr_image &in0, size_t inStride, const ovrfsr_image &out0, size_t outStride, uint32_t n);

// Can a recorded submission (fi -> fo) and the one that follows it (si -> so) go as ONE batch of two?  Image 1 lives at base + stride with
// the strides taken modulo 2^64 (the kernels add `i * stride` to a 64-bit base, i in {0, 1}): it may lie above or below image 0, inputs and
// outputs independently.  Images that differ in size / pitch / format, one texture submitted for both eyes, outputs that overlap an input
// or each other, or a stride that is no multiple of the texel size: no.
bool pairable(const ovrfsr_image &fi, const ovrfsr_image &fo, const ovrfsr_image &si, const ovrfsr_image &so, size_t *inStride, size_t *outStride);

struct Submission {
    int eye = 0;
    ovrfsr_image in = {}, out = {};
};

class SubmitSequencer {
public:
    enum class Action {
        Forward,     // no stage selected: the input is handed back
        Reuse,       // the second Submit of a shared side-by-side texture: the previous output
        Record,      // a frame's first eye: nothing launched, `out` is where its result will be
        LaunchPair,  // image 0 = the recorded eye, image 1 = this one, one batch of two
        LaunchSingle
    };
    // The steps of one Apply, in order; a step that fails ends the call (nothing further is reported to the sequencer).
    struct Steps {
        bool flush = false;      // first: `flushed` alone (the recorded submission whose other eye did not follow); then FlushDone()
        Submission flushed;
        Action action = Action::LaunchSingle;
        uint32_t images = 0;     // then: the images to launch -- 2 (LaunchPair), 1 (LaunchSingle) or none
        Submission launch;       // LaunchPair: image 0 and its eye, with the strides below; LaunchSingle: the image and the eye the kernels take
        size_t inStride = 0, outStride = 0;
        Submission current;      // this call's submission (Finish reads it)
        bool sameEyeAgain = false; // (FlushDone reads it)
    };
    // Called once the destination is accepted; writes what the call changes BEFORE its launches.
    Steps Begin(int eye, const ovrfsr_image &in, const ovrfsr_image &dst, bool pairMode, bool stages, bool onlyOneEye);
    void FlushDone(const Steps &s); // the flush step succeeded
    ovrfsr_image Finish(const Steps &s); // the action succeeded (or launched nothing): what the call changes AFTER it; -> the image the caller gets

    // "A recorded submission, if any, must go first" (a batch call, a change of the input size, a ctx-owned output that would have to grow
    // under it): hands it over and forgets it.
    bool TakeRecorded(Submission *s);
    // forgetOrder: an explicit reset forgets the learned submission order; the implicit one of a size change keeps it where it keeps the
    // ctx-owned image the flushed eye was handed in (PostProcessor::ResetKeeping)
    void Reset(bool forgetOrder);
    bool PairPending() const { return s_.lastApplyRecorded && s_.havePending; }

    struct State {
        // PostProcessor.h:66-68
        uintptr_t lastSubmittedTexture = 0;
        ovrfsr_image outputTexture = {};
        int eyeCount = 0;
        // cfg.pair_submit: the recorded FIRST submission of the current frame (either eye; see the header) and what it takes to launch it
        bool havePending = false;
        int pendingEye = 0;
        ovrfsr_image pendingIn = {}, pendingOut = {};
        int pairFirstEye = -1;          // the eye that opens a frame, learned from the last completed pair (-1: not known yet)
        bool pairDefer = true;          // false after the same eye came twice in a row, until the other eye is seen again
        int lastEye = -1;
        bool lastApplyRecorded = false; // the last Apply only recorded its submission (ovrfsr_pair_pending)
    };
    const State &state() const { return s_; }

private:
    State s_;
};

} // namespace ovrfsr
