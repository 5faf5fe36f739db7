// pipeline_plan.h -- what the launch manager will do for one (configuration, submitted format, size), decided on the host before anything is
// built on the device.  plan_pipeline() is pure: no HIP call, no device, no state -- footprints, mask classification, tile lists, LDS fit and
// every refusal are host arithmetic.  PostProcessor (postprocessor.cpp) plans, then uploads what the Plan holds; tests/debug/plan_probe.cpp
// runs the planner alone, under the host sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "../../include/openvr_fsr_amd.h"
#include "fsr_params.h"
#include "nis_tables.h"

namespace ovrfsr {

// host-side constant math (restates FsrEasuCon / FsrRcasCon / NVScalerUpdateConfig; see constants.cpp)
void easu_con(uint32_t con[16], float inVpW, float inVpH, float inW, float inH, float outW, float outH);
void rcas_con(uint32_t con[4], float stops);
void mask_constants(uint32_t centre[4], uint32_t radius[4], uint32_t outW, uint32_t outH, const float proj[4],
                    float cfgRadius, int onlyOneEye, int eye);
uint32_t classify_mask(const uint32_t centre[4], uint32_t r2, uint32_t outW, uint32_t outH, uint32_t gw, uint32_t gh);

// The launches of one apply, by the names the documents use ("Plan, then upload")
enum class Form {
    None,              // no stage selected: the submission is handed back untouched
    UpscaleOnly,       // EASU or NVScaler into the destination
    SharpenOnly,       // RCAS or NVSharpen (output size == input size)
    TwoPass,           // upscale into the intermediate, sharpen into the destination
    MaskSorted,        // masked EASU+RCAS: both passes on the tiles touching the radius, outside tiles written in final form (ApplySorted)
    Fused,             // one kernel, the intermediate in LDS
    FusedMaskedOutside // the fused kernel on the tiles touching the radius, outside tiles written in final form
};
const char *form_name(Form f); // for tests/debug/plan_probe.cpp: the library itself never prints a form

// OVRFSR_OK, or why the call is refused.  `disables`: refused like a failed build -- the ctx stays disabled until reset.
struct Refusal {
    int status = OVRFSR_OK;
    const char *text = "";
    bool disables = false;
    explicit operator bool() const { return status != OVRFSR_OK; }
};
// every refusal plan_pipeline and destination_refusal can produce, and nothing else they return.  Listed for tests/debug/plan_probe.cpp
// (tests/test_pipeline_plan.py holds the same list); the library does not call it.
const Refusal *plan_refusals(size_t *count);

// The tiles a launch's workgroups walk and the mask groups the radius is tested on, for one output size.  EASU, RCAS, the fused kernel and
// NVSharpen: 32x32 tiles (EASU: four of the 16x16 groups the reference dispatches); NVScaler: one workgroup per 32x24 mask group.  Everything
// that counts, lists or launches tiles reads this -- tile_lists, hidden_tiles' caller, the launch arguments, ovrfsr_hidden_area_stats.
struct TileGrid {
    uint32_t tileW = 0, tileH = 0;
    uint32_t groupW = 0, groupH = 0;
    uint32_t tx = 0, ty = 0;     // tiles per row, tile rows
    uint32_t tiles() const { return tx * ty; }
};
TileGrid tile_grid(bool useNis, bool doUpscale, uint32_t outW, uint32_t outH);

// Everything of a Plan but its tables: plain values, copied freely (the re-aim step hands back a Plan without the tap tables)
struct PlanFields {
    // what was planned for: the canonical submitted format (a multisampled encoding included), its size, one eye per texture or both
    uint32_t inputWidth = 0, inputHeight = 0, inputFormat = 0;
    bool onlyOneEye = true;
    uint32_t outputWidth = 0, outputHeight = 0;
    // stage selection, PostProcessor.cpp:530-535 / :586-594
    bool doUpscale = false, doSharpen = false;
    bool useNis = false;         // NVScaler / NVSharpen in place of EASU / RCAS
    Form form = Form::None;
    bool tileLists = false;      // the launches walk the per-eye tile lists below: product arithmetic, an upscale stage, and a mixed mask
                                 // (maskLists) or a hidden-area mesh (hiddenArea)
    bool maskLists = false;      // ... because of the mask: what tileLists is without a mesh.  The form is chosen from this one alone
    bool hiddenArea = false;     // a hidden-area mesh is in effect (HiddenArea): hidden tiles are in no list but the ring; the strict build,
                                 // sharpen-only forms and anything without an upscale stage ignore the mesh
    bool overlapOutside = false; // ... and their outside-tile kernel runs on the ctx's auxiliary stream (see PostProcessor::Fork)
    bool hdrDomain = false;      // OVRFSR_HDR_DOMAIN_SRTM is in effect (plan_pipeline, `hdrDomain`): everything here but inputFormat and
                                 // ownedFormat is the plan of the RGBA32F submission; the forward and back passes run around it
    // pipeline: what the kernels see in the submission's place; intermediate: the upscale stage's destination in front of a sharpen stage;
    // owned: the textures the ctx creates for itself (cfg.reference_formats)
    uint32_t pipelineFormat = 0, intermediateFormat = 0, ownedFormat = 0;
    // OVRFSR_PRECISION_FP32_EXACT is the product build everywhere but in RCAS: every launcher and size rule sees launchPrec, launch_rcas rcasPrec
    int launchPrec = PREC_FP32, rcasPrec = PREC_FP32;
    // "constant buffers", one per eye: PostProcessor.cpp:296-338, :419-460
    uint32_t easuCon[16] = {};
    uint32_t rcasCon[4] = {};
    NisConstants nis = {};       // the 256-byte NISConfig (PostProcessor.cpp:307-310)
    uint32_t centre[2][4] = {};
    uint32_t radius[4] = {};
    uint32_t maskMode[2] = {};
    float tieHalfMin = 0.0f;     // near-tie guard of a half intermediate (plan_pipeline); +inf = off
    float unorm8StoreGuard = 0.0f; // guard SWITCH of EASU's UNORM8 store of a float source (easu_tie_half_min): +inf = off, finite = on
    int cellsW = 0, cellsH = 0;           // LDS footprint of one EASU tile
    int fusedCellsW = 0, fusedCellsH = 0; // ... of the 34x34 EASU block of the fused kernel
    int nisCellsW = 0, nisCellsH = 0;     // ... of one 32x24 NVScaler group
    float rcpOut[2] = {0, 0};    // RN(1/outW), RN(1/outH) and whether mul+2fma reproduces o/out for every o (div_exact)
    bool rcpExact = false;
    // bilinear fallback / DirectCopy taps (Plan::taps): [outW column taps, padded to a multiple of the tile width with copies of the last |
    // outH row taps at tapYOff | 64 spare entries]
    uint32_t tapYOff = 0;
    uint32_t outsideCols = 0, outsideRows[2] = {0, 0}; // bilinear footprint bound of a 32-wide tile; rows for 32- and 24-row tiles
    // the tile grid of the output: what the launches' tilesX / tilesY are, what the lists below index
    TileGrid grid;
    // the tile lists, per eye: Plan::lists holds inside | ring | outside (| rcas) -- the ring tiles follow the inside tiles so that ONE EASU
    // launch over nInside + nRing entries also writes the intermediate of the ring, while RCAS walks the inside tiles only (ring: tiles
    // 4-adjacent to a tile RCAS processes whose intermediate no other launch writes); one 4-dword record per list entry
    // (OutsideArgs::tileRec); RCAS segments of the runs RCAS walks, 2 dwords each (RcasArgs::spanRec): Plan::lists, recs, spans
    uint32_t nInside[2] = {0, 0}, nOutside[2] = {0, 0}, nRing[2] = {0, 0}, nSpans[2] = {0, 0};
    size_t listOffInside[2] = {0, 0}, listOffOutside[2] = {0, 0}, listOffRing[2] = {0, 0}, spanOff[2] = {0, 0}; // spanOff in segments
    // what RCAS walks: the inside segment itself, or (two-pass under a hidden-area mesh) a fourth segment of its own -- every tile that is
    // not hidden, inside | outside merged in raster order -- and the spans are cut from it
    uint32_t nRcas[2] = {0, 0};
    size_t listOffRcas[2] = {0, 0};
    uint32_t nSkipped[2] = {0, 0}; // hiddenArea: tiles no launch writes the destination of (a hidden ring tile is still a skipped one)
    bool listsShared = false;    // both eyes have identical lists
    // A gaze-capable plan (plan_pipeline, `gaze`): the lists and the spans live in fixed per-eye regions sized for the worst case of any gaze, so
    // that reaim_pipeline's result fits where the current lists are -- eye e's lists start at e * listRegion (entries), its segments at
    // e * spanRegion (segments); what a region does not use is zero.  maskGroupW / H: the groups classify_mask tests the radius on.
    bool gazeCapable = false;
    size_t listRegion = 0, spanRegion = 0;
    uint32_t maskGroupW = 0, maskGroupH = 0;
    // A rescale-capable plan (plan_pipeline, `rescale`; header, "Dynamic resolution"): planned in the gaze layout above -- the lists stay
    // resident in their regions and tile_records_kernel addresses every entry's record --, so that rescale_pipeline's result needs nothing
    // but new constants, new tap tables and a records pass
    bool rescaleCapable = false;
};

struct Plan : PlanFields {
    std::vector<BilinTap> taps;
    std::vector<uint32_t> lists, recs, spans; // (PostProcessor frees these three once they are uploaded; the counts and offsets stay)
};

// ovrfsr_set_hidden_area's meshes as the planner takes them: per eye, `triangles` triangles of 3 x (u, v) floats (header: the rule)
struct HiddenArea {
    const float *uv[2] = {nullptr, nullptr};
    uint32_t triangles[2] = {0, 0};
};
// The classification rule (header, ovrfsr_hidden_tiles): hidden[tileY * tilesX + tileX] = 1 where every pixel of (tile & image) is covered by
// some triangle.  Integer arithmetic throughout; cost follows the triangles' bounding boxes.  With `right` (a shared side-by-side texture)
// `left` maps onto columns [0, outW / 2) and `right` onto [outW / 2, outW), each pixel tested against the mesh of its own half only.
void hidden_tiles(const float *left, uint32_t leftTriangles, const float *right, uint32_t rightTriangles, bool shared, uint32_t outW, uint32_t outH,
                  uint32_t tileW, uint32_t tileH, uint8_t *hidden);

// per eye, a byte per tile of the grid (hidden_tiles); empty: no mesh in effect
struct HiddenMaps {
    std::vector<uint8_t> eye[2];
};

// what tile_record (tile_records.h) computes a plan's records from, on the host (outside_records) and on the device (tile_records_kernel)
TileRecordGrid record_grid(const PlanFields &p);

// ovrfsr_output_size behind its argument checks
int plan_output_size(const ovrfsr_config &cfg, uint32_t inW, uint32_t inH, uint32_t *outW, uint32_t *outH);

// `format`: canonical (a single-sample encoding reduced to its base format).  On a refusal *plan is left as it was.
// `hidden`: the ctx's hidden-area meshes, or null (none set): the plan is then what it has always been.
// `hdrDomain`: ovrfsr_set_hdr_domain's value.  OVRFSR_HDR_DOMAIN_SRTM with a float pipeline format (RGBA16F, RGBA32F, R11G11B10F, any sample
// count) plans the pipeline of the RGBA32F submission of that size into an RGBA32F destination -- form, intermediate, mask, tile lists --,
// without the mesh (the back pass walks whole images), and RCAS in the launch precision (no UNORM8 byte leaves RCAS, so exact stores have
// nothing to guard there).  Plan::inputFormat stays the submission's and Plan::ownedFormat follows the submission's own rule.  Where the
// submission plans and its RGBA32F twin does not (a footprint only the half kernels' LDS planes hold), the setting is not applied.  UNORM
// formats and OVRFSR_HDR_DOMAIN_LINEAR: the plan is what it has always been.
// `gaze`: non-null plans a GAZE-CAPABLE plan (a gaze is set on either eye: ovrfsr_set_gaze; `cfg` is the effective configuration, the gazes
// in proj_centre) -- the same plan in every field but the list and span offsets, laid out in per-eye regions (PlanFields::gazeCapable) --
// and leaves the rasterised hidden-area maps there for reaim_pipeline.
// `rescale`: non-null plans a RESCALE-CAPABLE plan (a maximum input size is set: ovrfsr_set_max_input_size) -- the same plan in every field
// the kernels read, in the gaze layout whether or not a gaze is set (PlanFields::rescaleCapable), the maps left there like `gaze`'s.
Refusal plan_pipeline(const ovrfsr_config &cfg, uint32_t format, uint32_t width, uint32_t height, bool onlyOneEye, Plan *plan,
                      const HiddenArea *hidden = nullptr, int hdrDomain = OVRFSR_HDR_DOMAIN_LINEAR, HiddenMaps *gaze = nullptr,
                      HiddenMaps *rescale = nullptr);

// The re-aim step (header, "Eye-tracked foveation"): what becomes of `current` when only proj_centre moved -- `effective` is the configuration
// `current` was planned from with the gazes of the moment in proj_centre, `hidden` what plan_pipeline left in `gaze`.  Pure; re-runs
// mask_constants, classify_mask and steps 1-5 of the tile lists, never the mesh rasteriser, the footprints or the tap tables.
//   Nothing   the mask centres are the current ones: *reaimed is not written
//   InPlace   plan_pipeline(effective) differs from `current` in centre, maskMode, the lists, records and spans with their counts, nSkipped and
//             listsShared only, and the new lists fit the regions: *reaimed is that plan without its tap tables (`current` keeps them), and,
//             with `hostRecords` = false, without the records (the launch manager builds them on the device: tile_records_kernel)
//   Rebuild   anything else would move -- maskLists and with it the form, tileLists or overlapOutside; whether every group of both eyes is
//             inside the radius, which resolve_in_staging decides by; or `current` is not gaze-capable: plan afresh.  *reaimed is not written
enum class Reaim { Nothing, InPlace, Rebuild };
Reaim reaim_pipeline(const Plan &current, const ovrfsr_config &effective, const HiddenMaps &hidden, Plan *reaimed, bool hostRecords = true);

// The re-scale step (header, "Dynamic resolution"): what becomes of `current` when only the input size moved -- `effective` and `hdrDomain`
// are what `current` was planned from, `hidden` what plan_pipeline left in `rescale` (the lists stay, so the maps are not read).  Pure; re-runs
// the constants, the footprints, the refusals, the form rule and the tap tables for the new size, never the mesh rasteriser, reciprocals,
// the mask classification or the tile lists.
//   Nothing   the size is the planned one: *rescaled is not written
//   InPlace   plan_pipeline at the new size differs from `current` in inputWidth / inputHeight, easuCon, cells*, fusedCells*, nis, nisCells*,
//             the tap tables with outsideCols / outsideRows and the records only: *rescaled is that plan -- with the lists, spans and
//             host-built records where `current` still holds its lists, else without the three (the launch manager's lists are on the
//             device, where tile_records_kernel rebuilds the records)
//   Rebuild   anything else would move (the output size, doUpscale, the form, tileLists, maskLists, overlapOutside, a format), the fresh plan
//             is a refusal, or `current` is not rescale-capable: plan afresh.  *rescaled is not written
enum class Rescale { Nothing, InPlace, Rebuild };
Rescale rescale_pipeline(const Plan &current, const ovrfsr_config &effective, uint32_t width, uint32_t height, const HiddenMaps &hidden,
                         int hdrDomain, Plan *rescaled);

// what depends on the destination the call names
Refusal destination_refusal(const Plan &plan, uint32_t destFormat);
// EasuArgs::tieHalfMin of one EASU launch from inFormat into outFormat.  `halfGuard`: the guard of a half store (Plan::tieHalfMin, or the
// override an audit build puts in its place).
float easu_tie_half_min(const Plan &plan, uint32_t inFormat, uint32_t outFormat, float halfGuard);
// a 4-sample RGBA8 submission resolved, or a single-sample R11G11B10F one decoded, inside the kernels' staging instead of the resolve pass:
// the pipeline then reads the submission itself (its format, pitch and stride), and no ctx-owned copy exists
bool resolve_in_staging(const Plan &plan, uint32_t destFormat);

} // namespace ovrfsr
