// postprocessor.hpp -- HIP stream/launch manager that replaces the reference's D3D11 host pipeline
// (src/postprocess/PostProcessor.{h,cpp}).  Same public shape -- Apply(eye, texture, bounds) and
// Reset() -- same lazy (re)build rules, same stage selection; D3D11 resources become linear device
// buffers and `context->Dispatch` becomes a kernel launch on a caller-provided HIP stream.
#pragma once
#include <hip/hip_runtime_api.h>
#include <string>
#include <vector>
#include "../../include/openvr_fsr_amd.h"
#include "fsr_params.h"
#include "nis_tables.h"
#include "fsr_sizes.h"
#include "pipeline_plan.h"
#include "submit_sequence.h"

namespace ovrfsr {

#ifdef OVRFSR_BOUNDS
void debug_fail_resource(int nth); // checked builds: the nth device allocation / stream / event creation from now on fails, once (postprocessor.cpp)
void debug_tap_route(int upload);  // checked builds: a re-scale refills the tap tables by upload (1) or by tap_tables_kernel (0), from now on
#endif

// a device allocation that knows its size
struct DeviceBuffer {
    void *p = nullptr;
    size_t bytes = 0;
    void release();
};
struct DeviceGuard; // hipSetDevice for the duration of a call (postprocessor.cpp)

class PostProcessor {
public:
    PostProcessor(int device, const ovrfsr_config &cfg);
    ~PostProcessor();

    // PostProcessor::Apply, PostProcessor.cpp:123-164
    int Apply(int eye, const ovrfsr_image *in, const ovrfsr_bounds *bounds, ovrfsr_image *out, hipStream_t stream);
    int ApplyBatch(uint32_t n, int firstEye, int alternate, const ovrfsr_image *in0, size_t inStride,
                   const ovrfsr_image *out0, size_t outStride, hipStream_t stream, bool sharedTextures = false);
    // PostProcessor::Reset, PostProcessor.cpp:166-194
    void Reset();
    int SetConfig(const ovrfsr_config &cfg);
    const ovrfsr_config &GetConfig() const { return cfg_; }
    const char *LastError() const { return lastError_.c_str(); }
    bool PairPending() const { return sequence_.PairPending(); }
    // ovrfsr_set_hidden_area / ovrfsr_hidden_area_stats behind their argument checks
    int SetHiddenArea(int eye, const float *uv, uint32_t triangles);
    int HiddenAreaStats(int eye, uint32_t *tilesTotal, uint32_t *tilesSkipped);
    // ovrfsr_set_hdr_domain / ovrfsr_get_hdr_domain behind their argument checks
    int SetHdrDomain(int domain);
    int HdrDomain() const { return hdrDomain_; }
    // ovrfsr_set_gaze / ovrfsr_clear_gaze / ovrfsr_get_gaze / ovrfsr_gaze_stats behind their argument checks.  The setters store and nothing else:
    // the apply that launches the eye reads the value (EnsurePlanned -> AimGaze)
    void SetGaze(int eye, float x, float y);
    void ClearGaze(int eye);
    void GetGaze(int eye, float xy[2], int *isSet) const;
    void GazeStats(uint32_t *reaims, uint32_t *rebuilds) const { *reaims = reaims_; *rebuilds = rebuilds_; }
    // ovrfsr_set_max_input_size / ovrfsr_get_max_input_size / ovrfsr_rescale_stats behind their argument checks.  The setter stores the value
    // and does what SetHdrDomain does: the next apply plans afresh, rescale-capable where a maximum is set (EnsurePlanned -> RescaleInput)
    int SetMaxInputSize(uint32_t width, uint32_t height);
    void MaxInputSize(uint32_t *width, uint32_t *height) const { *width = maxInput_[0]; *height = maxInput_[1]; }
    void RescaleStats(uint32_t *rescales, uint32_t *rebuilds) const { *rescales = rescales_; *rebuilds = sizeRebuilds_; }
    // ovrfsr_set_mask_feather / ovrfsr_get_mask_feather / ovrfsr_mask_feather_stats behind their argument checks.  The setter stores and
    // nothing else, like SetGaze: the apply that launches reads the value (ApplyPostProcess -> ApplyFeather)
    void SetMaskFeather(float width) { feather_ = width; }
    float MaskFeather() const { return feather_; }
    uint32_t MaskFeatherLaunches() const { return featherLaunches_; }
#ifdef OVRFSR_BOUNDS
    int DebugReadTaps(void *dst, size_t bytes); // checked builds: the device tap tables as they are once the stream work so far is done
#endif
    int LastGpuTimeMs(float *ms);
    int AverageGpuTimeMs(float *ms, uint32_t *reports);

private:
    // What one apply hands from function to function, as values (plain aggregates: nothing computed, nothing owned).
    // A call: what every launch of one apply shares.
    struct Call { uint32_t n; int firstEye; int alternate; hipStream_t stream; };
    // An image run: image 0 of a call's n images and the byte distance to the next one -- taken modulo 2^64 (at_offset, postprocessor.cpp);
    // a run of one image has stride 0.
    struct ImageRun {
        ovrfsr_image first;
        size_t stride;
        // the tight run in `data`: images of w x h texels of `format`, rows `pitch` bytes apart, image after image
        static ImageRun Tight(void *data, uint32_t format, uint32_t w, uint32_t h, uint32_t pitch) { return {{data, w, h, pitch, format}, (size_t)pitch * h}; }
    };
    // What is asked for: the (canonical) image 0 of the submission, and whether its images hold one eye each.  compareEyeLayout: a batch call
    // also asks whether the plan assumes the same (Apply does not: PostProcessor::PlannedFor)
    struct Asked { ovrfsr_image in; bool onlyOneEye; bool compareEyeLayout; };
    static BatchView make_view(const ImageRun &from, const ImageRun &to); // what the kernels take of the two runs

    int device_;
    ovrfsr_config cfg_;
    std::string lastError_;
    std::vector<float> hiddenUv_[2]; // the hidden-area mesh of each eye, 6 floats per triangle: outlives Reset and SetConfig (header)
    int hdrDomain_ = OVRFSR_HDR_DOMAIN_LINEAR; // ovrfsr_set_hdr_domain's value: outlives Reset and SetConfig too
    // ovrfsr_set_gaze's values, per eye: they outlive Reset and SetConfig as well.  gazeMoved_: a setter was called since the plan was last
    // aimed -- the next apply asks the planner's re-aim step what that means (nothing, new lists in place, or a rebuild) and counts the answer
    bool gazeSet_[2] = {false, false};
    float gaze_[2][2] = {{0, 0}, {0, 0}};
    bool gazeMoved_ = false;
    uint32_t reaims_ = 0, rebuilds_ = 0;
    ovrfsr_config EffectiveConfig() const; // cfg_ with the gazes that are set in proj_centre: what the plan is made from
    // ovrfsr_set_max_input_size's value ({0, 0}: none): outlives Reset and SetConfig like the three above.  With one set the plan is
    // rescale-capable (Plan::rescaleCapable) and the buffers sized by the input are sized by the maximum.  rescales_ / sizeRebuilds_: the
    // applies whose input size differed from the planned one and that re-scaled in place / rebuilt, since create
    uint32_t maxInput_[2] = {0, 0};
    uint32_t rescales_ = 0, sizeRebuilds_ = 0;
    // ovrfsr_set_mask_feather's value (0: off), in cfg.radius's unit: outlives Reset and SetConfig like the four above, and touches no plan
    // -- the pass behind the pipeline reads it with the mask constants of the moment.  featherLaunches_: launches of that pass since create
    float feather_ = 0.0f;
    uint32_t featherLaunches_ = 0;

    // PostProcessor.h:16-24
    bool enabled_ = true;
    bool initialized_ = false;
    // what each Apply does with its submission -- the reference's Submit bookkeeping (PostProcessor.h:66-68) and the deferred pair of
    // cfg.pair_submit: decided on the host (submit_sequence.h); Apply launches what it is told
    SubmitSequencer sequence_;

    // What the ctx does for the current (configuration, submitted format, size): decided on the host (pipeline_plan.h), read by every
    // per-call helper.  A Reset replaces it with a fresh one.
    Plan plan_;
    // the plan's tables on the device (PrepareResources uploads them, in this order)
    float *nisCoefDev_ = nullptr;         // coef_scale[512] | coef_usm[512] (PostProcessor.cpp:366-381)
    BilinTap *bilinDev_ = nullptr;        // Plan::taps
    uint32_t *tileListDev_ = nullptr;     // Plan::lists, then inside the same allocation:
    uint32_t *tileRecDev_ = nullptr;      //   Plan::recs, 4 dwords per list entry
    uint32_t *spanRecDev_ = nullptr;      //   Plan::spans, 2 dwords per segment
    // under a hidden-area mesh that skips a tile: per eye, one bit per tile of the grid (bit t of word t / 32: tile t is hidden), for the
    // mask-feather pass, which neither reads nor writes such a tile.  The mesh decides it alone: a re-aim or a re-scale leaves it as it is
    uint32_t *hiddenBitsDev_ = nullptr;   // eye 0's words, then eye 1's
    int BuildHiddenBits(const HiddenArea &mesh);
    // A gaze-capable plan (Plan::gazeCapable): the same three tables laid out in the plan's per-eye regions, the records built on the device
    // (tile_records_kernel), and what a re-aim needs to put new lists there without a host wait: the hidden-area maps the planner rasterised,
    // and a ring of pinned staging slots, each a host image of the lists and spans (lists | spans, the device layout), each guarded by an
    // event that is recorded behind its copies and waited on before the slot is written again
    static constexpr int kGazeSlots = 4;
    HiddenMaps hiddenMaps_;
    uint32_t *gazeStage_ = nullptr;       // kGazeSlots x GazeSlotDwords() dwords of pinned host memory
    hipEvent_t gazeEvent_[kGazeSlots] = {};
    bool gazeSlotUsed_[kGazeSlots] = {};
    int gazeSlot_ = 0;
#ifdef OVRFSR_GAZE_HOST_RECORDS /* measurement build (never shipped): the records built on the host and uploaded behind the lists, no
                                  tile_records_kernel -- the other side of the comparison in profiles/gaze.txt */
    static constexpr bool kGazeHostRecords = true;
#else
    static constexpr bool kGazeHostRecords = false;
#endif
    // (a rescale-capable plan: the tap tables behind them, for the upload route of a re-scale -- 2 dwords per tap)
    size_t GazeSlotTapsAt() const { return (kGazeHostRecords ? 10 : 2) * plan_.listRegion + 4 * plan_.spanRegion; }
    size_t GazeSlotDwords() const { return GazeSlotTapsAt() + (plan_.rescaleCapable ? 2 * plan_.taps.size() : 0); }
#ifdef OVRFSR_RESCALE_UPLOAD_TAPS /* measurement build (never shipped): a re-scale uploads the host-built tap tables through a staging slot
                                     instead of running tap_tables_kernel -- the other side of the comparison in profiles/dynamic_resolution.txt */
    static constexpr bool kRescaleUploadTaps = true;
#else
    static constexpr bool kRescaleUploadTaps = false;
#endif
    void FreeTables();                    // the plan's tables on the device and the staging ring
    int BuildFailed(hipError_t e, const char *what); // a creation or upload of PrepareResources failed
    int BuildStagingRing();                           // the pinned ring and its events
    int BuildGazeTables(hipStream_t stream);          // PrepareResources' part for the tile lists of a gaze-capable plan
    TileRecordsArgs RecordsArgs() const;              // tile_records_kernel over every list entry in use
    // EnsurePlanned's re-scale step (header, "Dynamic resolution"): is this input the planned one at another size, on a ctx with a maximum?
    // Then *step is the planner's answer and, for InPlace, *rescaled the plan RescaleInPlace puts in plan_'s place
    bool SizeMoved(const Asked &asked) const;
    int RescaleInPlace(Plan &rescaled, hipStream_t stream);
    // one image of a ctx-owned copy of the input (resolved_, swizzled_, hdrIn_: input_copy_bytes, fsr_sizes.h) for a submission of
    // (format, w, h) -- or, where that is more, for the maximum input size: what a rescale-capable ctx allocates, so that no later size within
    // the maximum grows it.  PrepareResources asks with the maximum itself
    size_t SizedForMax(InputCopy copy, uint32_t format, uint32_t w, uint32_t h) const
    {
        const uint64_t now = input_copy_bytes(copy, format, w, h), atMax = plan_.rescaleCapable ? input_copy_bytes(copy, format, maxInput_[0], maxInput_[1]) : 0;
        return (size_t)(atMax > now ? atMax : now);
    }
    int UploadGazeLists(const Plan &from, hipStream_t stream); // lists and spans through the next staging slot, then the records
    int AimGaze(hipStream_t stream);      // EnsurePlanned's gaze step: nothing, a re-aim in place, or a rebuild of the tables
    // the memory-bound outside-tile kernel and the VALU-bound inside-tile kernel are independent: the former runs on
    // a ctx-owned auxiliary stream, forked from and joined back into the caller's stream with events
    hipStream_t auxStream_ = nullptr;
    hipEvent_t evFork_ = nullptr, evJoin_ = nullptr;
    bool replan_ = false;     // ovrfsr_set_hdr_domain asked for a fresh plan: no plan is "for" any input until the next apply has reset and rebuilt
    bool capturing_ = false;  // the stream of the call in progress is being captured into a HIP graph: launches only, no (re)build
    DeviceBuffer retired_;    // a ctx-owned output image a flushed pair_submit eye was handed in, kept across the rebuild of a size change
    void ResetKeeping(bool keepRetired);
    int FlushPending(hipStream_t stream, bool *ownedOutput = nullptr); // the recorded submission of cfg.pair_submit on its own, if there is one
    // What Apply and ApplyBatch do before they look at the destination: device, capture refusal, "is the plan still for this input", reset,
    // PrepareResources.  Their two deliberate differences are the last two arguments.
    enum class Recorded {
        GoesFirst,   // ApplyBatch: a recorded eye is launched before the size is looked at
        OnChange     // Apply: only where the plan changes, and a ctx-owned image it was handed in is retired, not freed
    };
    int EnsurePlanned(const DeviceGuard &guard, const Asked &asked, Recorded recorded, hipStream_t stream);
    bool PlannedFor(const Asked &asked) const;
    hipStream_t Fork(hipStream_t user, bool overlap);
    void Join(hipStream_t user, hipStream_t aux);

    // ctx-owned device buffers: upscaledTexture / sharpenedTexture, PostProcessor.h:43-45,58-59
    DeviceBuffer swizzled_;  // RGBA8 copy of a BGRA8 submission (tight pitch), see ApplyPostProcess
    DeviceBuffer resolved_;  // single-sample copy of a multisampled submission, RGBA16F copy of an R11G11B10F one that is not decoded in staging (rows padded to 16 B), see ApplyPostProcess
    DeviceBuffer upscaled_;
    DeviceBuffer sharpened_;
    DeviceBuffer hdrIn_, hdrOut_; // Plan::hdrDomain: the mapped RGBA32F copy the pipeline reads and the RGBA32F image it writes (tight rows, image after image), see ApplyPostProcess

    // debug-mode GPU timing, PostProcessor.h:72-82: a ring of kQueryCount timestamp pairs; after every apply the OLDEST
    // slot is read back (so the wait is normally over already), durations are summed and every 500 readings the mean
    // is published -- doubled when each eye has its own texture, i.e. "per frame" (PostProcessor.cpp:605-626)
    static constexpr int kQueryCount = 6;
    struct ProfileQuery { hipEvent_t start = nullptr, end = nullptr; bool pending = false; uint32_t images = 1; };
    ProfileQuery queries_[kQueryCount];
    int currentQuery_ = 0, lastQuery_ = -1;
    float summedGpuTime_ = 0.0f;   // seconds
    int countedQueries_ = 0;
    float avgGpuTimeMs_ = 0.0f;
    uint32_t avgReports_ = 0;
    void CollectQuery(hipStream_t stream);

    int Fail(int status, const std::string &what);
    int CheckImage(const ovrfsr_image *img, const char *name, bool input = false); // input: may be multisampled / R11G11B10F
    int PrepareResources(const Asked &asked, hipStream_t stream); // :498-561: plan (pipeline_plan.h), then upload
    // one masked launch round: images first, first + step, ... (cnt of them) of the batch, all of eye `eye` when `split`
    struct EyePass {
        int eye; uint32_t cnt, first, step; bool split;
        template <class Args> void Select(Args &a) const; // narrows an argument block of the whole batch (its view, its mask) to this pass
    };
    int EyePasses(const Call &call, EyePass out[2]) const;
    // body(const EyePass &, hipStream_t aux) -> hipError_t, once per pass, between Fork and Join; `what` names the launch in the error text.
    // `mayOverlap` = false: no fork -- aux is the caller's stream, and no event is recorded or waited on
    template <class Body> int ForEachEyePass(const Call &call, bool mayOverlap, const char *what, Body body);
    // one pass's two launches: `inside` with the list of the tiles touching the radius (+ `ring` tiles behind them) on the caller's stream,
    // then `outside` with the list and records of the other tiles on the auxiliary one
    template <class In, class Out, class LaunchIn, class LaunchOut>
    hipError_t InsideThenOutside(const EyePass &ps, In inside, Out outside, uint32_t ring, LaunchIn launchInside, LaunchOut launchOutside) const;
    const uint32_t *InsideList(int eye) const { return tileListDev_ + plan_.listOffInside[eye]; }
    const uint32_t *OutsideList(int eye) const { return tileListDev_ + plan_.listOffOutside[eye]; }
    const uint32_t *OutsideRecords(int eye) const { return tileRecDev_ + 4 * plan_.listOffOutside[eye]; }
    const uint32_t *RcasList(int eye) const { return tileListDev_ + plan_.listOffRcas[eye]; } // (the inside list, or RCAS's own: Plan::nRcas)
    const uint32_t *SpanRecords(int eye) const { return spanRecDev_ + 2 * plan_.spanOff[eye]; }
    void RcasOverList(RcasArgs &a, int eye) const; // RCAS on the tiles the plan lists for it (Plan::nRcas), by span records where it has them
    int Launched(hipError_t e, const char *what); // OVRFSR_OK, or OVRFSR_ERR_HIP with "<what> launch: <hip error>"
    template <class Args> void FillScale(Args &a, const ImageRun &in, const ImageRun &out, const Call &call) const;
    void FillRcas(RcasArgs &a, const ImageRun &in, const ImageRun &out, const Call &call) const;
    void FillEasu(EasuArgs &a, const ImageRun &in, const ImageRun &out, const Call &call) const;
    void FillNis(NisArgs &a, const ImageRun &in, const ImageRun &out, const Call &call) const; // (the view and the tile grid too)
    int EnsureBuffer(DeviceBuffer &buf, size_t need);
    int IntermediateImage(uint32_t n, ImageRun *mid); // the upscale stage's destination in front of a sharpening stage
    int RefuseDisablingDestination(uint32_t format);
    float TieHalfMin() const;
    // one apply: `submitted` -> `out`, the FINAL destination (:563-638), and its steps in order --
    int ApplyPostProcess(const Call &call, const ImageRun &submitted, const ImageRun &out);
    // the pipeline's input: the submission itself, or the resolve / unpack pass into resolved_, or the BGRA8 re-order into swizzled_
    // (starts the timer: in front of the resolve, behind the re-order)
    int PipelineInput(const Call &call, const ImageRun &submitted, uint32_t outFormat, bool timing, ImageRun *in);
    // the HDR wrap: the forward map of *in into hdrIn_, which takes its place, and the run in hdrOut_ in *out's (the back map follows the form)
    int HdrWrap(const Call &call, ImageRun *in, ImageRun *out);
    // the form switch; `mid`: the two-pass form's intermediate
    int ApplyForm(const Call &call, const ImageRun &in, const ImageRun &mid, const ImageRun &out);
    int ApplyUpscaling(const Call &call, const ImageRun &in, const ImageRun &out);  // :385-401
    int ApplySorted(const Call &call, const ImageRun &in, const ImageRun &out);
    int ApplyFused(const Call &call, const ImageRun &in, const ImageRun &out);
    int ApplySharpening(const Call &call, const ImageRun &in, const ImageRun &out); // :483-496
    // the mask-feather pass (header, "Mask feather") behind the form's launches: `in` the pipeline's input, `out` what the form wrote
    int ApplyFeather(const Call &call, const ImageRun &in, const ImageRun &out);
    void FillMask(MaskArgs &m, const Call &call) const;
};

} // namespace ovrfsr
