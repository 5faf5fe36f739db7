// submit_sequence.cpp -- see submit_sequence.h.  Reference: the Submit bookkeeping of src/postprocess/PostProcessor.cpp:153-163; the deferred
// pair of cfg.pair_submit has no counterpart there.
#include "submit_sequence.h"
#include "fsr_formats.h"

namespace ovrfsr {

static inline uintptr_t address(const ovrfsr_image &img) { return reinterpret_cast<uintptr_t>(img.data); }

bool ranges_overlap(const ovrfsr_image &in0, size_t inStride, const ovrfsr_image &out0, size_t outStride, uint32_t n)
{
    const uintptr_t i0 = address(in0), o0 = address(out0);
    const uintptr_t i1 = i0 + (n - 1) * inStride + (size_t)in0.pitch_bytes * in0.height;
    const uintptr_t o1 = o0 + (n - 1) * outStride + (size_t)out0.pitch_bytes * out0.height;
    return i0 < o1 && o0 < i1;
}

bool pairable(const ovrfsr_image &fi, const ovrfsr_image &fo, const ovrfsr_image &si, const ovrfsr_image &so, size_t *inStride, size_t *outStride)
{
    const bool same = fi.width == si.width && fi.height == si.height && fi.pitch_bytes == si.pitch_bytes && fi.format == si.format &&
                      fo.width == so.width && fo.height == so.height && fo.pitch_bytes == so.pitch_bytes && fo.format == so.format;
    // integer arithmetic on the addresses: the wrap of an unsigned difference is defined, `p - q` across objects is not
    *inStride = (size_t)(address(si) - address(fi));
    *outStride = (size_t)(address(so) - address(fo));
    const bool disjoint = fi.data != si.data && !ranges_overlap(fo, 0, so, 0, 1) && !ranges_overlap(fi, 0, so, 0, 1) && !ranges_overlap(si, 0, fo, 0, 1) &&
                          !ranges_overlap(fi, 0, fo, 0, 1) && !ranges_overlap(si, 0, so, 0, 1);
    return same && disjoint && *inStride % texel_bytes(fi.format) == 0 && *outStride % texel_bytes(fo.format) == 0;
}

bool SubmitSequencer::TakeRecorded(Submission *s)
{
    if (!s_.havePending) return false;
    s_.havePending = false;
    *s = Submission{s_.pendingEye, s_.pendingIn, s_.pendingOut};
    return true;
}

void SubmitSequencer::Reset(bool forgetOrder)
{
    const State fresh;
    State kept = fresh; // a recorded first eye of cfg.pair_submit is dropped (header)
    if (!forgetOrder) { kept.pairFirstEye = s_.pairFirstEye; kept.pairDefer = s_.pairDefer; kept.lastEye = s_.lastEye; }
    s_ = kept;
}

// Pairing is by ARRIVAL order (round 6: games submit L,R or R,L; until then only LEFT was recorded and an R,L game had every LEFT batched
// with the NEXT frame's RIGHT).  A small state machine keeps a disturbed sequence from turning into a standing one-frame lag:
//   recorded, other eye arrives  -> both as one batch of two; that pair's first eye is remembered as the frame's first eye
//   recorded, SAME eye again     -> the older one alone, this one alone, and no more recording until the other eye shows up
//                                   (a host that submits one eye per frame, or a frame that lost an eye)
//   nothing recorded             -> recorded if it is (or may be) a frame's first eye; a frame's SECOND eye with nothing recorded
//                                   (its partner was flushed by a batch call or a size change) is processed at once
SubmitSequencer::Steps SubmitSequencer::Begin(int eye, const ovrfsr_image &in, const ovrfsr_image &dst, bool pairMode, bool stages, bool onlyOneEye)
{
    Steps st;
    st.current = Submission{eye, in, dst};
    s_.lastApplyRecorded = false;
    if (pairMode) {
        const int prevEye = s_.lastEye;
        s_.lastEye = eye;
        if (s_.havePending && s_.pendingEye == eye) {
            st.flush = TakeRecorded(&st.flushed);
            st.sameEyeAgain = true; // then this eye alone
        } else if (s_.havePending) {
            s_.pairFirstEye = s_.pendingEye;
            s_.pairDefer = true;
            Submission first;
            (void)TakeRecorded(&first);
            if (pairable(first.in, first.out, in, dst, &st.inStride, &st.outStride)) {
                st.action = Action::LaunchPair;
                st.images = 2;
                st.launch = first;
                return st;
            }
            st.flush = true; // two single launches instead
            st.flushed = first;
        } else if (!s_.pairDefer) {
            if (prevEye >= 0 && prevEye != eye) s_.pairDefer = true; // both eyes are back: pairs again from the next call on
        } else if (s_.pairFirstEye < 0 || s_.pairFirstEye == eye) {
            st.action = Action::Record; // the first eye of a frame: recorded, and the caller is handed where its result will be
            return st;
        }
    }
    // a shared side-by-side texture is processed once, on the first Submit (:155-158)
    const bool processed = s_.eyeCount == 0 || onlyOneEye || address(in) != s_.lastSubmittedTexture;
    st.action = !processed ? Action::Reuse : stages ? Action::LaunchSingle : Action::Forward;
    st.images = st.action == Action::LaunchSingle ? 1 : 0;
    st.launch = Submission{onlyOneEye ? eye : OVRFSR_EYE_LEFT, in, dst};
    st.inStride = st.outStride = 0;
    return st;
}

void SubmitSequencer::FlushDone(const Steps &st)
{
    if (st.sameEyeAgain) s_.pairDefer = false;
}

ovrfsr_image SubmitSequencer::Finish(const Steps &st)
{
    switch (st.action) {
    case Action::Record:
        s_.pendingIn = st.current.in; s_.pendingOut = st.current.out; s_.pendingEye = st.current.eye; s_.havePending = true;
        s_.lastApplyRecorded = true;
        s_.outputTexture = st.current.out;
        break;
    case Action::LaunchPair:
    case Action::LaunchSingle:
        s_.outputTexture = st.current.out;
        break;
    case Action::Forward:
        s_.outputTexture = st.current.in;
        break;
    case Action::Reuse:
        break;
    }
    s_.lastSubmittedTexture = address(st.current.in);
    s_.eyeCount = (s_.eyeCount + 1) % 2;
    return s_.outputTexture;
}

} // namespace ovrfsr
