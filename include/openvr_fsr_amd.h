/*
 * openvr_fsr_amd.h -- C ABI of the MI355X-native per-eye upscaler (FSR1 EASU + RCAS, NIS).
 *
 * This is the drop-in boundary for the reference's post-process hot path: everything
 * vr::PostProcessor does between "game submitted an eye texture" and "upscaled texture handed to
 * the compositor" (reference: src/postprocess/PostProcessor.{h,cpp}), with the D3D11 compute
 * dispatches replaced by HIP kernels for gfx950.  Plain pointers and sizes only; no C++/torch
 * types.  All image pointers are DEVICE pointers (the reference's input is an ID3D11Texture2D
 * already resident on the GPU -- PostProcessor.cpp:133).  Nothing here throws; every entry point
 * returns an ovrfsr_status and leaves outputs untouched on failure (PostProcessor.cpp:145-152).
 *
 * Reference interface each declaration replaces is cited as file:line under /root/reference/.
 * The reference-side binding a maintainer would write is in INTEGRATION.md.
 */
#ifndef OPENVR_FSR_AMD_H
#define OPENVR_FSR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define OVRFSR_API __attribute__((visibility("default")))
#else
#define OVRFSR_API
#endif

#define OVRFSR_ABI_VERSION 5u /* 5: ovrfsr_pair_pending added; pair_submit pairs by arrival order; create / set_config validate the float fields (multisampled inputs, OVRFSR_FORMAT_MS, came later without a version change: probe with one, an older library refuses it as OVRFSR_ERR_UNSUPPORTED; the same holds for the input format OVRFSR_FORMAT_R11G11B10F = 6).  4: ovrfsr_config::pair_submit (was reserved[0]; same struct size).  3: ovrfsr_apply_batch_shared added.  2: ovrfsr_average_gpu_time_ms added; precision value 1 (never built) removed */

typedef enum ovrfsr_status {
    OVRFSR_OK = 0,
    OVRFSR_ERR_INVALID_ARGUMENT = 1, /* null / misaligned / inconsistent descriptor            */
    OVRFSR_ERR_UNSUPPORTED = 2,      /* format or scale the path does not cover                 */
    OVRFSR_ERR_HIP = 3,              /* a HIP runtime call failed; see ovrfsr_last_error()      */
    OVRFSR_ERR_NO_DEVICE = 4,        /* no gfx950 device / kernels not loadable                 */
    OVRFSR_ERR_DISABLED = 5,         /* ctx disabled itself after a failed (re)build, like
                                        PostProcessor::enabled=false (PostProcessor.cpp:148-151)*/
    OVRFSR_ERR_OUT_OF_MEMORY = 6
} ovrfsr_status;

/* vr::EVREye, headers/openvr.h:149-153 */
typedef enum ovrfsr_eye { OVRFSR_EYE_LEFT = 0, OVRFSR_EYE_RIGHT = 1 } ovrfsr_eye;

/* Pixel formats of the linear device buffers that stand in for ID3D11Texture2D.
 * RGBA8_UNORM is what the reference allocates for its outputs (DetermineOutputFormat,
 * PostProcessor.cpp:63-74); RGBA16F is the packed-half I/O of BASELINE config C5; RGBA32F exists
 * so that parity can be measured on un-quantised results.  RGB10A2_UNORM (DXGI_FORMAT_R10G10B10A2_UNORM
 * bit layout: R 0-9, G 10-19, B 20-29, A 30-31) is the other format DetermineOutputFormat returns: a
 * 10-bit submission keeps 10-bit intermediate and output textures.  It is accepted as input with a
 * RGB10A2 (or, for parity measurements, RGBA32F) output, two-kernel pipeline only (cfg.fused = 1 is
 * rejected for it).  BGRA8_UNORM is input-only: the B8G8R8A8 submissions the reference views through a
 * typed SRV (TranslateTypelessFormats / MakeSrgbFormatsTypeless, PostProcessor.cpp:30-61) while its own
 * textures stay R8G8B8A8; here the channels are re-ordered by a copy kernel in front of the pipeline and
 * everything after it is the RGBA8 path. */
typedef enum ovrfsr_format {
    OVRFSR_FORMAT_RGBA8_UNORM = 0,
    OVRFSR_FORMAT_RGBA16F = 1,
    OVRFSR_FORMAT_RGBA32F = 2,
    OVRFSR_FORMAT_RGB10A2_UNORM = 3,
    OVRFSR_FORMAT_BGRA8_UNORM = 4,
    /* 5 is unassigned and refused (OVRFSR_ERR_UNSUPPORTED), on purpose: the tests use it as their example of an unknown format.  Do not
     * renumber the next one to close the gap. */
    OVRFSR_FORMAT_R11G11B10F = 6
} ovrfsr_format;

/* R11G11B10F (DXGI_FORMAT_R11G11B10_FLOAT: Unity's DefaultHDR render target and a common scene-colour format elsewhere).  INPUT-ONLY.
 * One 32-bit word per texel: R in bits 0-10, G in bits 11-21, B in bits 22-31; 4-byte texels, data and pitch_bytes aligned to 4.  The
 * reference views such a texture with its own format (TranslateTypelessFormats: `default: return format`, PostProcessor.cpp:30-48,206-220),
 * lets the sampler decode it and writes R8G8B8A8_UNORM (:63-74).
 * Decode rule: each channel is an unsigned float with a 5-bit exponent of bias 15 and a 6-bit (R, G) or 5-bit (B) mantissa, which is a
 * half float without its sign bit and its low mantissa bits: channel = the half float whose bits are the channel's bits shifted left by
 * 4 (R, G) or 5 (B).  That is exact for every code: denormals, +Inf (exponent 31, mantissa 0) and NaN included; the largest finite values
 * are 65024 (R, G) and 64512 (B).  Alpha reads 1.0, as D3D11 defines for a missing channel (the filters never read it).
 * The decode runs where the product build's EASU, fused and outside-tile kernels stage or load their texels (a single-sample submission on
 * a path with an upscale stage: no pass, no copy) and otherwise in the resolve pass in front of the pipeline, into a ctx-owned RGBA16F copy
 * (multisampled submissions, the strict build, NIS, sharpen-only, tile footprints wider than 40 texels); everything behind it is the RGBA16F
 * pipeline: an R11G11B10F submission gives, byte for byte, what the RGBA16F image holding the same values (alpha 1.0) gives, on every
 * path and in every build -- same intermediate choices, same tolerances, same texel-value domain (no negative values exist; Inf and NaN
 * codes fall under the texel-value clause below: outside the parity contract, inside the memory-safety one).  Destinations: those of
 * an RGBA16F input (RGBA8, RGBA16F, RGBA32F); a ctx-owned output (out->data == NULL) is RGBA16F -- RGBA8, through a UNORM8 intermediate,
 * with cfg.reference_formats = 1, which is what the reference does with such a texture.  As an `out`, and for ovrfsr_save_ppm /
 * ovrfsr_save_dds: OVRFSR_ERR_UNSUPPORTED (the float -> float11 rounding is left to the implementation by D3D, and the reference never
 * writes the format); the ctx stays enabled.  OVRFSR_FORMAT_MS(OVRFSR_FORMAT_R11G11B10F, S), S = 2, 4, 8, is accepted with the
 * multisampled layout below and the float resolve rule applied to the decoded samples (fp32 sum in sample order, times 1/S, half
 * rounded to nearest even), in the same pass.  cfg.fsr_enabled = 0 forwards the descriptor untouched.  A library older than this format
 * refuses it as OVRFSR_ERR_UNSUPPORTED: that is how a host probes for it, the ABI version is unchanged.  What the pass costs where it
 * remains, and a step without it: profiles/r11g11b10f_c5.txt, profiles/r11g11b10f_in_place.txt. */

/* MULTISAMPLED INPUT (D3D11_TEXTURE2D_DESC::SampleDesc.Count > 1; the reference resolves such a texture into a single-sample copy of
 * the input's own format before filtering: PrepareResources / GetInputView, PostProcessor.cpp:196-224,520-523).  The sample count
 * travels in the high bits of ovrfsr_image::format: OVRFSR_FORMAT_MS(OVRFSR_FORMAT_RGBA8_UNORM, 4).  Samples 0 or 1 = single-sample;
 * 2, 4 and 8 are accepted for every base format, for INPUT images only (a multisampled `out`, ovrfsr_save_ppm / ovrfsr_save_dds of
 * one: OVRFSR_ERR_UNSUPPORTED); any other count or bit: OVRFSR_ERR_UNSUPPORTED.  A library older than this feature refuses every such
 * value as an unknown format (OVRFSR_ERR_UNSUPPORTED): that is how a host probes for it, the ABI version is unchanged.
 * Layout: samples interleaved per texel -- sample s of texel (x, y) at data + y*pitch_bytes + (x*S + s)*texel_bytes;
 * pitch_bytes >= width*S*texel_bytes; alignment that of the base format; the 4 GiB span rule applies to the multisampled image.
 * Resolve rule (D3D11 leaves resolve rounding to the implementation; this is the stated choice, the same in every build and
 * precision), into the input's base format: UNORM channels (8-bit; RGB10A2's 10-bit RGB and 2-bit A) (sum_i k_i + S/2) >> log2 S in
 * integers; RGBA16F / RGBA32F decoded to fp32, summed in sample order s0 + s1 + ... (no contraction, no re-association), multiplied by
 * 1/S, half rounded to nearest even.  The result is what "resolve, then apply to the single-sample image" gives, bit for bit, on every
 * path.  4x RGBA8 input on an unmasked product-build EASU pass with a UNORM8 destination (the two-kernel pipeline's intermediate, or an
 * EASU-only UNORM8 output: C2's path) is resolved inside EASU's staging sweep, with the same integer rule, so nothing extra is written;
 * every other multisampled input -- other formats and counts, masked / mask-sorted, cfg.fused = 1, NIS, RCAS-only, the strict build --
 * takes a resolve kernel that writes a ctx-owned single-sample copy (BGRA8 re-ordered in the same pass) for the pipeline to run on.  A change
 * of sample count is a format change (rebuild; refused under capture).  cfg.fsr_enabled = 0 forwards the multisampled descriptor
 * untouched.  The debug-mode timer (ovrfsr_last_gpu_time_ms) includes the resolve, where the reference starts its query after
 * ResolveSubresource (PostProcessor.cpp:574-581): where the resolve is fused into EASU's staging it cannot be timed apart, so the figure
 * is the cost of the whole path from the submitted texture on every path. */
#define OVRFSR_FORMAT_SAMPLES_SHIFT 8
#define OVRFSR_FORMAT_MS(fmt, samples) ((uint32_t)(fmt) | ((uint32_t)(samples) << OVRFSR_FORMAT_SAMPLES_SHIFT))

/* Arithmetic the kernels run in.  The reference only ever compiles the fp32 bodies
 * (`//#define A_HALF`, src/fsr/fsr_easu.hlsl:3).
 *   FP32         fp32 math, FMA contraction allowed, hardware rcp (<= 1 ulp): the product build.  Its quantised EASU stores (the UNORM8 /
 *                half intermediate of a pipeline, an EASU-only UNORM8 output) are nevertheless the STRICT build's, bit for bit: a pixel whose
 *                re-associated result lies within 2^-9 byte of a UNORM8 rounding boundary -- for half stores within 2^-6 of a half spacing,
 *                that band scaled with the largest texel of the tile's input footprint where it exceeds 1 (HDR: the re-association error
 *                follows the largest tap, not the output), for values >= xmin = 0.25 / 0.5 derived from the sharpness (a flipped half-ulp
 *                below xmin stays under 1e-3 behind RCAS's largest gain) -- is re-resolved in the reference's operator order (near-tie
 *                guard).  This is AUDITED, not derived: an audit build of the same kernels (-DOVRFSR_TIE_AUDIT) re-resolves every
 *                pixel in reference order on the device and counts the unlisted pixels whose stored value differs -- 0 in 1.2e12 pixels over
 *                every configuration, structured / random / extreme / natural content, RGBA16F content up to 40x the unit range, and the
 *                candidates of a directed search that maximises the distance between the two evaluations; the largest distance met is
 *                3.5e-4 byte, 0.18 of the band (profiles/r05_tie_audit.txt, profiles/r06_tie_audit_campaigns.txt,
 *                tests/test_gpu_adversarial.py).  A first-order worst-case bound of that distance is
 *                two orders of magnitude above the band (same file, section 5): the filter's one ill-conditioned step, the direction blend, is
 *                evaluated in the reference's order for that reason, the rest is rounding noise that no norm bound captures.  A violation,
 *                should one exist, is one LSB (one half-ulp) of one intermediate pixel.  Float outputs differ by <= 3e-6, UNORM8 pipeline
 *                outputs by <= 1 LSB, half pipeline outputs by <= 1e-3 on unit-range images and by <= one half-ulp of the value beyond
 *   FP32_STRICT  fp32, every operator evaluated as written (no FMA), IEEE division: bit-identical
 *                to the CPU oracle; a validation build, not a fast one
 * Pixels OUTSIDE the radius (the reference's `Bilinear` fallback, fsr_easu.hlsl:33-36, and NIS `DirectCopy`, NIS_Upscale.hlsl:77-90 --
 * 78 % of a frame at the shipped radius 0.5) and NVScaler's chroma tap are one SampleLevel through D3D11's default linear-clamp sampler.
 * Both builds evaluate it as the D3D11 functional spec describes that sampler -- texel coordinate snapped to 8 fractional bits, round to
 * nearest, weights applied unfused -- and are bit-identical to the oracle there.  That reading is a restatement of the spec, not of anything
 * in the reference (it is fixed-function hardware), so its exposure is stated instead of its proof (profiles/r06_sampler_exposure.txt): if
 * hardware keeps MORE sub-texel bits (10, 12, exact float weights), pixels outside the radius move by <= 1 LSB -- none at all at BASELINE's
 * C2 / C3 shape, whose scale is exactly 3/4 (every coordinate a multiple of 1/4), 1.9 % of the bytes at x1.3 (C4 shape) on structured and
 * natural content, 10.8 % on uniform noise; a TRUNCATING snap would move 0.6 % / 3.9 % of them by <= 2 LSB.
 * TEXEL VALUES the statements above cover (tests/test_gpu_formats.py::test_texel_value_domain; for NVScaler / NVSharpen
 * tests/test_gpu_nis_formats.py::test_nis_texel_value_domain): every finite value whose fp32 products do
 * not overflow -- the whole RGBA16F range, negative values, denormals, RGBA32F magnitudes up to 1e18.  One thing IEEE 754 leaves open shows
 * through: min / max of a +0 and a -0.  An image holding zeros of BOTH signs can make a result that is a zero carry the other sign than the
 * oracle's (x86 and gfx950 choose differently); colour images (values >= +0) never meet it.  NaN / +-Inf texels, and magnitudes whose products
 * overflow (1e30), are outside the parity contract and inside the memory-safety one: what the pixels whose taps reach such a texel hold is
 * implementation-defined (EASU / RCAS: the same pixels are NaN in every build and in the oracle), every other pixel is unaffected, nothing is
 * read or written out of place (checked build, profiles/r06_bounds.txt).
 * There is no packed-half arithmetic mode (value 1 was reserved for one in ABI 1 and is rejected with
 * OVRFSR_ERR_INVALID_ARGUMENT by ovrfsr_create / ovrfsr_set_config): on gfx950 v_pk_*_f16 issues at the rate of
 * v_pk_*_f32 (profiles/r02_valu_issue_rates.txt), the fp32 kernels already process two taps per packed instruction, and
 * half accumulation of 12 taps misses the 1e-3 tolerance (measured: 3.9e-3, profiles/r03_half_acc.txt) -- the "fp16" of BASELINE configs C2/C3/C5 is served by fp32
 * arithmetic with RGBA16F images and a half intermediate where the config asks for packed-half I/O.
 *   FP32_EXACT   exact stores.  Arithmetic, kernels, tile lists, launch forms and tolerances are FP32's; in addition every UNORM8 byte the
 *                pipeline stores is the STRICT build's.  EASU's bytes are that already (above); here RCAS gets the same kind of guard on the
 *                final byte: a pixel with a channel within 2^-11 byte of a rounding boundary is evaluated a second time in the reference's
 *                operator order and stored with the reference's rounding (profiles/exact_stores.txt; audited like the
 *                EASU guard).  Covered: every pipeline whose RCAS reads an RGBA8 intermediate or input and writes RGBA8 -- unmasked and
 *                masked EASU+RCAS, RCAS-only, shared textures, batches, pair_submit, BGRA8 and multisampled RGBA8 submissions, float /
 *                R11G11B10F submissions under reference_formats = 1; EASU-only passes and pixels outside the radius go through as in FP32.
 *                Refused at (re)build with OVRFSR_ERR_UNSUPPORTED (ctx disabled until ovrfsr_reset, the caller's image untouched): use_nis,
 *                fused = 1, quantize_intermediate = 0 in front of RCAS, and an RCAS whose source or destination is not RGBA8 (half / float /
 *                RGB10A2 intermediates, inputs or `out` images).  Added without an ABI version change: a host probes with ovrfsr_create and
 *                precision = 3, which a library from before this value answers with OVRFSR_ERR_INVALID_ARGUMENT. */
typedef enum ovrfsr_precision {
    OVRFSR_PRECISION_FP32 = 0,
    OVRFSR_PRECISION_FP32_STRICT = 2,
    OVRFSR_PRECISION_FP32_EXACT = 3
} ovrfsr_precision;

/* Stands in for vr::Texture_t{handle,eType,eColorSpace} (headers/openvr.h:177-182) plus the
 * D3D11_TEXTURE2D_DESC the reference queries from the handle (PostProcessor.cpp:137-139). */
typedef struct ovrfsr_image {
    void *data;           /* device pointer to texel (0,0); aligned to the texel size (4 / 8 / 16 B)    */
    uint32_t width;       /* texels                                                              */
    uint32_t height;      /* texels                                                              */
    uint32_t pitch_bytes; /* distance between rows; multiple of the texel size; >= width*texel   */
    uint32_t format;      /* ovrfsr_format; inputs: | samples << OVRFSR_FORMAT_SAMPLES_SHIFT     */
} ovrfsr_image;

/* vr::VRTextureBounds_t, headers/openvr.h:609-613.  Only |uMax-uMin| > 0.5 is consulted
 * ("texture contains only one eye", PostProcessor.cpp:146). */
typedef struct ovrfsr_bounds { float uMin, vMin, uMax, vMax; } ovrfsr_bounds;

/* The numeric fields of the reference's Config singleton that reach the GPU
 * (src/postprocess/Config.h:10-17), plus the values the reference obtains from the OpenVR runtime
 * (projection centres, PostProcessor.cpp:104-121) and implementation knobs of this library.
 *
 * Configuration values.  The mask centre and radius are float expressions converted to uint32 (PostProcessor.cpp:298-305); the
 * reference validates nothing -- its one rule is `if (sharpness < 0) sharpness = 0` (Config.h:40) -- and that conversion is undefined
 * behaviour in C++ for NaN, negative or huge values.  This library never evaluates it on such a value:
 *   - ovrfsr_create / ovrfsr_set_config return OVRFSR_ERR_INVALID_ARGUMENT (no ctx is built / the old cfg stays) for a radius that is
 *     not finite or is negative, a sharpness or render_scale that is not finite, or a proj_centre component outside [-1, 2] (or NaN);
 *   - sharpness is otherwise clamped to [0, 1] where the reference clamps it (PostProcessor.cpp:420, NIS_Config.h);
 *   - ovrfsr_mask_constants is total: for 0 <= x < 2^32 the conversion is the reference's truncation (every known answer holds), NaN
 *     and negative values give 0, values >= 2^32 give 0xffffffff (the saturating float->uint of the shader model that reads the
 *     cbuffer); radius^2 keeps the reference's uint32 wrap-around (radius * outH / 2 >= 65536: defined, if useless, there too);
 *   - ovrfsr_config_from_json clamps a negative radius to 0 exactly as the reference clamps a negative sharpness, and treats a
 *     number that overflows float as "Could not read config file" (defaults, OVRFSR_ERR_INVALID_ARGUMENT); numbers are read in the "C"
 *     locale whatever locale the host process has set (a comma-decimal LC_NUMERIC would make atof("0.77") return 0). */
typedef struct ovrfsr_config {
    uint32_t struct_size;    /* = sizeof(ovrfsr_config); ABI guard                               */
    int32_t fsr_enabled;     /* Config::fsrEnabled: 0 -> apply() is a pass-through (output = input
                                handle untouched, PostProcessor.cpp:135)                         */
    int32_t use_nis;         /* Config::useNis.  DEPARTURE FROM THE REFERENCE, NVScaler only: the reference ignores
                                NVScalerUpdateConfig's `false` for a scale outside [0.5, 1] (in/out; i.e. upscales
                                beyond 2x, or any render_scale > 1) and dispatches with a half-initialised NISConfig
                                block (PostProcessor.cpp:308, NIS_Config.h:144-160: the result is undefined).  Here
                                such a configuration fails the (re)build: ovrfsr_apply* returns
                                OVRFSR_ERR_UNSUPPORTED, the ctx disables itself like any failed PrepareResources
                                (PostProcessor.cpp:148-151) and the caller's texture goes through untouched       */
    int32_t debug_mode;      /* Config::debugMode: tints pixels outside the radius               */
    float render_scale;      /* Config::renderScale; <1: out = in / scale, >=1: out = in * scale,
                                both truncated to uint (PostProcessor.cpp:512-518)               */
    float sharpness;         /* Config::sharpness, [0,1] (clamped where the reference clamps)    */
    float radius;            /* Config::radius, in units of outH/2; 2.0 disables the mask; finite, >= 0 */
    float proj_centre[4];    /* {Lx, Ly, Rx, Ry} in [0,1]: what CalculateProjectionCenter()
                                returned for each eye; default 0.5; accepted range [-1, 2]       */
    uint32_t out_width;      /* explicit output size; 0,0 = derive from render_scale             */
    uint32_t out_height;
    int32_t precision;       /* ovrfsr_precision                                                 */
    int32_t quantize_intermediate; /* 1 = EASU result is stored as UNORM8 before RCAS reads it,
                                as the reference's R8G8B8A8_UNORM intermediate texture does
                                (PostProcessor.cpp:348); 0 = intermediate kept in float          */
    int32_t fused;           /* 0 two kernels through an HBM intermediate, 1 one kernel with the
                                intermediate in LDS (same results for the same quantize_intermediate
                                up to the product build's rounding), -1 auto: whichever is faster
                                for the configuration (two kernels unmasked; with a radius mask the
                                tiles outside the radius are written in final form by a concurrent
                                kernel and the tiles touching it take the two-kernel form for RGBA8
                                pipelines, the fused one for half / float)                       */
    int32_t stage_mask;      /* 0 = the reference's stage selection (upscale iff scale != 1, sharpen
                                iff !use_nis || scale == 1; PostProcessor.cpp:586-594).  1 = upscale
                                stage only (BASELINE config C1 "EASU-only"), 2 = sharpen stage only  */
    int32_t pair_submit;     /* 0 = every ovrfsr_apply processes its eye at once: the reference's pattern, two dispatches per Submit,
                                four dependent launches per frame (PostProcessor.cpp:586-594).
                                1 = deferred pair, for submissions with one texture per eye: the ovrfsr_apply of the FIRST eye of a frame
                                -- LEFT or RIGHT, games submit in either order -- only RECORDS the submission and returns, in *out, the
                                image that eye's result will be written to (ovrfsr_pair_pending() then returns 1); the ovrfsr_apply of
                                the OTHER eye then launches BOTH as one batch of two -- two launches per frame.  The first eye's output is complete, in stream order, once the
                                second call has returned: a host must hold back whatever consumes it (the forwarded Submit,
                                INTEGRATION.md) until then, and the first eye's INPUT texture must stay unmodified until then too (it is
                                read when the pair is launched, not when it is recorded).  Same pixels, bit for bit.
                                One frame costs 0.097 instead of 0.110 ms of GPU time at 1683x1869 -> 2244x2492 (ramp-up, the partly
                                filled last round of workgroups and the drain are paid per launch), 0.05 instead of 0.07 ms at the
                                shipped radius 0.5.  The two images of a pair may sit anywhere in memory relative to each other (inputs
                                and outputs independently).  A recorded eye whose other eye does not follow -- the same eye again, a
                                texture of another size or format, one texture submitted for both eyes, outputs that overlap,
                                ovrfsr_apply_batch* -- is processed on its own by that next call.  A disturbed sequence does not become
                                a standing lag: after the same eye twice in a row nothing is recorded until the other eye is seen again
                                (a host that submits ONE eye per frame pays one late result, once), and a frame's second eye that finds
                                nothing recorded (its partner went out with a batch call or a size change) is processed at once; only a
                                host that REVERSES its eye order mid-stream should call ovrfsr_reset.  ovrfsr_reset /
                                ovrfsr_set_config / ovrfsr_destroy DROP a recorded eye and forget the learned order.  Both eyes must get their own output image:
                                caller-owned ones, or the two ctx-owned images of this mode (a ctx-owned image handed out for a recorded
                                eye stays valid across the rebuild a size change triggers, until the next reset)                */
    int32_t reference_formats; /* (was reserved[0]; same struct size, ABI version unchanged)
                                0 = the default, THIS LIBRARY'S OWN rule (BASELINE C5, packed-half I/O): the intermediate and a ctx-owned
                                output have the format of the pipeline's input -- an RGBA16F / R11G11B10F submission runs through a half
                                intermediate and comes back as RGBA16F, an RGBA32F one as RGBA32F.
                                1 = THE REFERENCE'S rule: both of its own textures are created in DetermineOutputFormat(input)
                                (PostProcessor.cpp:63-74, 340-352, 462-475): R10G10B10A2_UNORM for a 10-bit submission, R8G8B8A8_UNORM for
                                everything else, RGBA16F, RGBA32F and R11G11B10F included.  With quantize_intermediate = 1 the
                                intermediate, and in any case the ctx-owned output (out->data == NULL, both ctx-owned images of
                                pair_submit), are RGBA8 for a float submission: EASU writes a saturating UNORM8 intermediate, RCAS
                                sharpens bytes (strict build: bit-identical to the oracle's composition; product build: <= 1 LSB, and the
                                UNORM8 EASU store of a float source is the strict build's bit for bit -- near-tie guard with the band
                                2^-9 byte x max(1, largest texel of the tile's footprint), audited: profiles/reference_formats.txt).
                                A caller-owned `out` keeps selecting the final store conversion (an RGBA32F `out` still serves parity
                                measurements); quantize_intermediate = 0 keeps its fp32 intermediate, only the ctx-owned output's format
                                follows the rule.  For RGBA8, BGRA8 and RGB10A2 inputs the field changes nothing.  cfg.fused = 1 with
                                the rule and a float pipeline input fails the (re)build with OVRFSR_ERR_UNSUPPORTED, like RGB10A2 (no
                                fused kernel is built for a byte intermediate of a float source); fused = -1 takes the mask-sorted
                                two-kernel form there.  Values other than 0 and 1: OVRFSR_ERR_INVALID_ARGUMENT.  A library older than this
                                field ignores it (reserved was never validated): a host probes by submitting a float image with
                                out->data == NULL and reading out->format.  The config-file parser does not set it (the reference has no
                                such key)                                                                                        */
    int32_t reserved[1];
} ovrfsr_config;

typedef struct ovrfsr_ctx ovrfsr_ctx; /* one per device; not thread-safe; distinct ctxs are independent */

/* Config.h:10-17 defaults (fsrEnabled=false, renderScale=1, sharpness=0.75, radius=0.5), centres 0.5 */
OVRFSR_API void ovrfsr_config_default(ovrfsr_config *cfg);

/* Stands in for the implicit construction of the global `postProcessor` (VrHooks.cpp:19) +
 * Config::Instance().  `device` is a HIP device ordinal. */
OVRFSR_API int ovrfsr_create(int device, const ovrfsr_config *cfg, ovrfsr_ctx **out_ctx);
OVRFSR_API void ovrfsr_destroy(ovrfsr_ctx *ctx);

/* What the reference's hotkeys do: mutate Config then Reset() (PostProcessor.cpp:659-709). */
OVRFSR_API int ovrfsr_set_config(ovrfsr_ctx *ctx, const ovrfsr_config *cfg);
OVRFSR_API int ovrfsr_get_config(const ovrfsr_ctx *ctx, ovrfsr_config *cfg);

/* PostProcessor::Reset() (PostProcessor.h:13, .cpp:166-194): drop cached constants and ctx-owned
 * resources, re-enable after a failure. */
OVRFSR_API int ovrfsr_reset(ovrfsr_ctx *ctx);

/* Output size rule of PrepareResources (PostProcessor.cpp:512-518). */
OVRFSR_API int ovrfsr_output_size(const ovrfsr_config *cfg, uint32_t in_width, uint32_t in_height,
                                  uint32_t *out_width, uint32_t *out_height);

/* PostProcessor::Apply(EVREye, const Texture_t*, const VRTextureBounds_t*, EVRSubmitFlags)
 * (PostProcessor.h:12, .cpp:123-164).
 *   in      the submitted eye texture (or the shared side-by-side texture).
 *   bounds  may be NULL (= {0,0,1,1}, PostProcessor.cpp:128-131).
 *   out     in/out.  If out->data is NULL the ctx-owned output image is used and *out is filled in
 *           -- the reference's behaviour of swapping Texture_t::handle for its own texture
 *           (PostProcessor.cpp:161), valid until the next apply on this ctx.  If out->data is set
 *           the result is written there (width/height must equal the output size; format
 *           selects the store conversion; its bytes must not overlap the input image's: the sharpen
 *           stages read neighbour texels other workgroups write -- OVRFSR_ERR_INVALID_ARGUMENT).  When the ctx is a pass-through (fsr disabled, or the
 *           second Submit of a shared texture, PostProcessor.cpp:155-158) *out describes the
 *           image the compositor should receive and nothing is launched.
 *   stream  hipStream_t (NULL = default stream).  Launches are asynchronous on it.  A ctx owns scratch device
 *           memory (the EASU->RCAS intermediate, its output image) and an auxiliary stream that is forked from
 *           and joined back into `stream` with events: consecutive calls on one ctx must be ordered by the
 *           caller -- same stream, or synchronised streams -- exactly like draws on one D3D11 immediate context.
 *           After the first call for a given input size a call allocates nothing and can be captured into a
 *           HIP graph.  A call that WOULD have to build something while `stream` is being captured (the first call for an
 *           input size, a larger batch than any before, the first use of the ctx-owned output) is refused with
 *           OVRFSR_ERR_INVALID_ARGUMENT before it touches anything -- the capture stays valid, the ctx stays enabled: make
 *           the same call once outside the capture.  A captured call records no debug-mode timestamps.
 * (Re)builds constants on first use and whenever the input size changes (PostProcessor.cpp:136-153). */
OVRFSR_API int ovrfsr_apply(ovrfsr_ctx *ctx, int eye, const ovrfsr_image *in, const ovrfsr_bounds *bounds,
                            ovrfsr_image *out, void *stream);

/* Batch form for headless throughput: n eye images of identical shape, image i at
 * base + i*stride_bytes, one launch over the whole batch.  Eye of image i is
 * first_eye ^ (alternate_eyes ? (i & 1) : 0): a batch of stereo pairs is laid out L,R,L,R,...
 * Each image is its own texture (textureContainsOnlyOneEye), outputs are caller-owned and must not overlap the inputs. */
OVRFSR_API int ovrfsr_apply_batch(ovrfsr_ctx *ctx, uint32_t n, int first_eye, int alternate_eyes,
                                  const ovrfsr_image *in0, size_t in_stride_bytes,
                                  const ovrfsr_image *out0, size_t out_stride_bytes, void *stream);

/* The same for SHARED side-by-side textures -- one image holds both eyes, what games that submit a single texture with
 * half-width bounds do (|uMax-uMin| <= 0.5, PostProcessor.cpp:146): every image is processed once with the two mask
 * centres of the shared layout (imageCentre of the left eye and width/2 * (1 + projX_R) for the right one,
 * PostProcessor.cpp:155-158,298-301), exactly as the first ovrfsr_apply of such a texture does. */
OVRFSR_API int ovrfsr_apply_batch_shared(ovrfsr_ctx *ctx, uint32_t n, const ovrfsr_image *in0, size_t in_stride_bytes,
                                         const ovrfsr_image *out0, size_t out_stride_bytes, void *stream);

OVRFSR_API const char *ovrfsr_last_error(const ovrfsr_ctx *ctx);

/* Averaged GPU time of the launches of the last apply, like the debug-mode timestamp queries
 * (PostProcessor.cpp:579-628).  Blocks until that work is done.  Only recorded when
 * cfg.debug_mode != 0. */
OVRFSR_API int ovrfsr_last_gpu_time_ms(ovrfsr_ctx *ctx, float *ms);

/* The reference's debug-mode log line "Average GPU processing time for upscale" (PostProcessor.cpp:605-626): a ring of
 * 6 timestamp pairs, the oldest read back after every apply, the mean of 500 readings published -- doubled when each eye
 * has its own texture (one reading = one eye, the figure = one frame).  *ms = the last published mean (0 before the
 * first), *reports = how many have been published; with OVRFSR_LOG=1 in the environment each one is also printed to
 * stderr in the reference's wording.  Only recorded when cfg.debug_mode != 0. */
OVRFSR_API int ovrfsr_average_gpu_time_ms(ovrfsr_ctx *ctx, float *ms, uint32_t *reports);

/* cfg.pair_submit (ABI 5): 1 when the most recent ovrfsr_apply on this ctx only RECORDED its submission (nothing was launched for it; its
 * output image will be complete once the next ovrfsr_apply has returned), 0 otherwise (also for a NULL ctx and with pair_submit off).
 * What a Submit detour needs to decide whether to hold the forwarded Submit back.  The reference has no counterpart:
 * it processes every eye inside its own Submit (VrHooks.cpp:50-62). */
OVRFSR_API int ovrfsr_pair_pending(const ovrfsr_ctx *ctx);

/* ---- hidden-area mesh: tiles the headset never shows are not processed ---------------------------
 * A VR runtime knows, per eye, which parts of the eye image no lens ever shows: IVRSystem::GetHiddenAreaMesh(eye,
 * k_eHiddenAreaMesh_Standard) lists them as triangles.  With a mesh set, the plan sorts the 32x32 output tiles (NVScaler: 32x24 groups)
 * that lie ENTIRELY inside the hidden area out of its tile lists on the host, and no launch touches them.  The reference has no
 * counterpart (its radius mask saves the expensive filter, never the pixel).  No ABI change: a host probes for these symbols.
 *
 * The rule, in integer arithmetic (the same on every host and in any restatement).  For an image of W x H output pixels:
 *   vertex       u and v are clamped to [-4, 4] in double; X = (int64)floor(u*W*256 + 0.5), Y = (int64)floor(v*H*256 + 0.5).
 *                v = 0 is the first stored row (a runtime whose v origin is at the bottom passes 1 - v).
 *   pixel        the centre of pixel (x, y) is (256x + 128, 256y + 128).
 *   coverage     with the three edge functions in int64: a triangle of zero area covers nothing; any other covers the pixel iff all three
 *                are >= 0 or all three are <= 0 -- either winding, edges inclusive.
 *   hidden       a pixel is hidden iff some triangle of its eye's mesh covers it; a tile iff every pixel of (tile & image) is hidden.
 *   shared side-by-side textures (both eyes in one image), W2 = W / 2: the left mesh maps onto columns [0, W2), the right mesh onto
 *                [W2, W) (X = floor(u * width of that half * 256 + 0.5) + 256 * its first column); a pixel is tested against the mesh
 *                of its own half only.
 * Contract:
 *   - for every pixel outside a skipped tile the result is bit-identical to the same call with no mesh set -- in every form and format,
 *     for batches, shared textures and pair_submit;
 *   - pixels of skipped tiles are NOT WRITTEN: a caller-owned `out` keeps its bytes there; the ctx-owned output image is zero-filled
 *     once, when it is allocated while a mesh is set;
 *   - a skipped tile is always a hidden tile.  Which hidden tiles are skipped is the plan's choice per form, reported by
 *     ovrfsr_hidden_area_stats: every hidden tile wherever the plan walks tile lists -- product arithmetic (OVRFSR_PRECISION_FP32 and
 *     FP32_EXACT) with an upscale stage: EASU-only, two-pass, mask-sorted, fused, fused with outside tiles, NVScaler --, none in the
 *     strict build, in the sharpen-only forms (RCAS or NVSharpen alone) and for a float submission under OVRFSR_HDR_DOMAIN_SRTM (below: its
 *     back pass walks whole images).  The front passes (multisample resolve, BGRA8 re-order,
 *     R11G11B10F unpack) run on the whole image.  (In the two-kernel forms EASU still writes the INTERMEDIATE of a hidden tile that
 *     shares an edge with a tile RCAS processes: RCAS's cross taps read it.  The destination is not written there.) */

/* Set (or, with triangle_count = 0, clear; uv may then be NULL) one eye's mesh: triangles as GetHiddenAreaMesh returns them, 3 vertices x
 * (u, v) per triangle, u, v in [0,1] of ONE eye's image; coordinates outside [0,1] are legal and clipped by the rule.  The mesh is copied.
 * Like ovrfsr_set_config it drops a recorded pair_submit eye and makes the next apply rebuild (refused under stream capture, as any
 * build is); ovrfsr_reset and ovrfsr_set_config keep the mesh, ovrfsr_destroy frees it.  OVRFSR_ERR_INVALID_ARGUMENT -- the stored mesh
 * is left as it was -- for a NULL ctx, an eye other than 0 or 1, a non-finite coordinate, uv == NULL with a count, more than 4096 triangles. */
OVRFSR_API int ovrfsr_set_hidden_area(ovrfsr_ctx *ctx, int eye, const float *uv, uint32_t triangle_count);
/* After a successful apply: the tiles per image of that eye's list (32x32; NVScaler 32x24), and how many of them the current plan skips
 * (0 wherever the plan ignores the mesh).  OVRFSR_ERR_INVALID_ARGUMENT before the first apply after a (re)build was asked for. */
OVRFSR_API int ovrfsr_hidden_area_stats(const ovrfsr_ctx *ctx, int eye, uint32_t *tiles_total, uint32_t *tiles_skipped);
/* Constants-only, no GPU: the classification rule itself, for known-answer tests and for a host that wants a preview.  One eye's mesh on
 * an out_w x out_h image (1..16384 each) cut into tile_w x tile_h tiles: hidden[tileY * ceil(out_w / tile_w) + tileX] = 1 for a hidden
 * tile, else 0.  hidden_len: bytes at `hidden`; too few (or any bad argument, checked as above): OVRFSR_ERR_INVALID_ARGUMENT, nothing written. */
OVRFSR_API int ovrfsr_hidden_tiles(const float *uv, uint32_t triangle_count, uint32_t out_w, uint32_t out_h,
                                   uint32_t tile_w, uint32_t tile_h, uint8_t *hidden, size_t hidden_len);

/* ---- HDR domain: float eye images are tone-mapped around the filters ---------------------------------------
 * ffx_fsr1.h states the input domain of EASU and RCAS as {0 to 1}: RCAS's limiter is built on a peak of 1.0 (it changes sign where a
 * neighbourhood's maximum exceeds 1), and EASU's edge analysis follows the largest tap, so one specular highlight of a few hundred decides
 * direction and length of the filter for every pixel around it.  The same header ships the answer, the Simple Reversible Tone-Mapper
 * (FsrSrtmF / FsrSrtmInvF, src/fsr/ffx_fsr1.h:1029-1046): linear HDR to {0 to 1} in front of the filters and back behind them, RGB ratios
 * preserved.  DEPARTURE FROM THE REFERENCE, opt-in: the reference filters linear HDR as it comes (and so does OVRFSR_HDR_DOMAIN_LINEAR, the
 * default: every byte is what it has always been).  No ABI change: a host probes for these symbols.
 *
 * The rule, in fp32, every operator rounded once as written, IEEE division, on the host (ovrfsr_hdr_map) and on the device alike:
 *   forward   m = max(max(r, g), b);  k = 1.0f / (m + 1.0f);                         r *= k; g *= k; b *= k
 *   back      m = max(max(r, g), b);  k = 1.0f / max(1.0f / 32768.0f, 1.0f - m);     r *= k; g *= k; b *= k
 * Alpha is not touched.  Covered values: finite and >= 0 (no ordering question about max arises for them); negative, NaN and Inf texels
 * fall under the texel-value clause above: outside the parity contract, inside the memory-safety one.  The round trip is NOT the
 * identity: forward rounds, and the back mapping's divisor is clamped, so it peaks at 32768 times the mapped value -- a texel beyond 32767
 * comes back as at most 32768, and a half destination (largest finite value 65504) holds whatever a mapped value <= 1 un-maps to.  The
 * filters can overshoot 1 in the mapped domain, though: RCAS's limiter bounds the lobe from the four cross taps, not the result, and on
 * noise between highlights the reference's own arithmetic (the CPU oracle) returns mapped values up to 2.6.  Such a value un-maps to 32768
 * times itself, and from 2 upwards that is past the half range: an RGBA16F destination then holds +Inf there, as the store conversion of
 * any value beyond 65504 does; an RGBA32F destination holds the finite product.
 *
 * The contract, with OVRFSR_HDR_DOMAIN_SRTM set and a submission whose pipeline format is float (RGBA16F, RGBA32F, R11G11B10F, single-sample
 * or OVRFSR_FORMAT_MS) -- a composition, bit for bit:
 *   1. the front pass runs where the submission needs one (multisample resolve, R11G11B10F unpack);
 *   2. a forward pass writes a ctx-owned single-sample RGBA32F copy holding the mapped values;
 *   3. the pipeline runs exactly as it is planned for an RGBA32F submission of that size with an RGBA32F destination -- form, intermediate,
 *      mask, NIS or FSR, reference_formats are that plan's -- into a second ctx-owned RGBA32F image;
 *   4. a back pass un-maps that image into the destination the call names, with that format's store conversion: RGBA32F as is, RGBA16F
 *      rounded to nearest even, RGBA8 saturate, x 255, + 0.5, truncate.
 * So the bytes equal: decode the submission to fp32, map, apply as an RGBA32F image into an RGBA32F `out` on a ctx without the setting,
 * un-map, convert.  The two mapped copies are fp32 on purpose: near m -> 1 the back mapping multiplies by 1 / (1 - m), and a half there
 * (spacing 2^-11) would turn a texel of 1000 into anything between 670 and 2000.
 *   - The format of a ctx-owned output (out->data == NULL) stays what it is for that submission: RGBA16F for half and R11G11B10F, RGBA32F for
 *     float, RGBA8 under cfg.reference_formats = 1.
 *   - UNORM submissions (RGBA8, BGRA8, RGB10A2) ignore the setting entirely: plans, launches and bytes are what they are without it.
 *   - Batches, shared side-by-side textures and pair_submit work like any other call; after the first call for a size nothing is allocated
 *     and the call can be captured; the debug-mode timer brackets the two passes, as it brackets the resolve.
 *   - A hidden-area mesh is IGNORED, as in the strict build and the sharpen-only forms: the back pass walks whole images, so nothing may be
 *     left unwritten; ovrfsr_hidden_area_stats reports 0 skipped tiles.
 *   - OVRFSR_PRECISION_FP32_EXACT: RCAS stores fp32 under this setting, no UNORM8 byte for exact stores to guard, so it runs as in
 *     OVRFSR_PRECISION_FP32 (EASU's UNORM8 intermediate under reference_formats = 1 is the strict build's in either).  What the submission is
 *     refused for without the setting it is refused for with it; nothing else is.  Where a submission plans and its RGBA32F twin would not
 *     (an LDS footprint only the half kernels hold: steep minification), the setting is not applied to that plan.
 * What it costs -- three more passes over 16-byte texels -- and what folding the mapping into the kernels' staging and stores would save:
 * profiles/hdr_domain.txt. */
#define OVRFSR_HDR_DOMAIN_LINEAR 0 /* the filters see the texel values as submitted: the default, and the reference's behaviour */
#define OVRFSR_HDR_DOMAIN_SRTM 1   /* float submissions are filtered in FSR 1's reversible tone-mapped domain */
/* OVRFSR_ERR_INVALID_ARGUMENT -- the stored value is left as it was -- for a NULL ctx or a value other than the two above.  Like
 * ovrfsr_set_hidden_area it drops a recorded pair_submit eye, re-enables a disabled ctx and makes the next apply rebuild (refused under stream
 * capture, as any build is).  The call itself touches no device resource -- what it retires is released by that next apply -- so it is
 * accepted while a stream is being captured and leaves the capture valid.  ovrfsr_reset and ovrfsr_set_config keep the value. */
OVRFSR_API int ovrfsr_set_hdr_domain(ovrfsr_ctx *ctx, int domain);
OVRFSR_API int ovrfsr_get_hdr_domain(const ovrfsr_ctx *ctx, int *domain);
/* Constants-only, no GPU: the mapping itself on n RGB triples (rgb_in and rgb_out: 3 * n floats; they may be the same array), forward
 * (inverse = 0) or back (inverse = 1).  OVRFSR_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer with n > 0 or any other `inverse`. */
OVRFSR_API int ovrfsr_hdr_map(const float *rgb_in, float *rgb_out, size_t n, int inverse);

/* ---- eye-tracked foveation: the radius mask follows the gaze, per frame ----------------------------------
 * cfg.proj_centre fixes the centre of the sharp disc per eye, as the reference does.  A headset with eye tracking wants the disc where the
 * eye looks, every frame; ovrfsr_set_config moves it too, but it is a reset: everything freed, re-planned and uploaded again.  A gaze moves
 * the centre and nothing else.  No ABI version and no config field changes with these: a host probes for the symbols.
 *
 * x, y: proj_centre's convention and range -- [0, 1] of ONE eye's image, y = 0 at the first stored row, accepted in [-1, 2].
 * Outside [0, 1] the centre is what ovrfsr_mask_constants makes of it: a negative coordinate is the coordinate 0 (the float -> uint store
 * saturates; the reference's cast is undefined there), one above 1 puts the centre behind the image's edge -- a sliver of the disc on the
 * image, or none of it: every pixel is then the bilinear fallback.  On a shared side-by-side texture a left gaze above 1 lands in the right
 * half.  Groups are inside or outside by the reference's per-group rule on the groups it dispatches, at every such centre
 * (tests/test_mask_edges.py, tests/test_gpu_mask_edges.py).
 *
 * THE RULE.  With a gaze set for eye e, every call behaves as the same call on a fresh ctx whose cfg.proj_centre holds the gaze in eye e's
 * two slots (the two centres of a shared side-by-side texture go through ovrfsr_mask_constants as they do today): status, error text,
 * the image handed back, every byte written, ovrfsr_hidden_area_stats -- in every form, format, build and precision, for batches (eye e's
 * gaze applies to every image of that eye), pair_submit, hidden-area meshes and OVRFSR_HDR_DOMAIN_SRTM.  ovrfsr_clear_gaze returns the eye
 * to cfg.proj_centre.  ovrfsr_reset and ovrfsr_set_config keep the gaze.
 *
 * LATCHING.  The gaze is read by the apply that launches the eye.  Unlike the other setters, ovrfsr_set_gaze drops no recorded pair_submit
 * eye, re-enables no disabled ctx and forces no rebuild by itself; a recorded pair launches with the gazes in effect at its SECOND call.
 * Set both eyes' gazes before the frame's first apply.
 *
 * WHAT AN APPLY AFTER A GAZE CHANGE DOES, one of three (ovrfsr_gaze_stats counts the second and the third):
 *   - nothing: the mask centres, integers in output pixels, are the current ones (0.5 -> 0.5001 at width 160);
 *   - a RE-AIM in place: only the centres, the per-eye mask modes and the tile lists move.  No allocation, no blocking copy, no host wait
 *     (the new lists go through a small ring of pinned staging slots on the call's stream; the host waits only where the host is more
 *     than the ring's four uploads ahead of the device), the ctx-owned output and intermediate images stay where they are;
 *   - a REBUILD of the ctx's tables: the mask moved between "mixed" and "no tile inside / every tile inside" (both gazes at (2, 2)), or the
 *     gaze was set on a ctx planned without one.  Sizes and formats do not move with a gaze, so the images the ctx owns and a recorded
 *     pair_submit eye keep their place; a rebuild that fails disables the ctx until reset, like any failed build, and one that runs out of
 *     memory answers OVRFSR_ERR_OUT_OF_MEMORY.
 * Under stream capture the setter is accepted; an apply that would re-aim or rebuild is refused like any build (OVRFSR_ERR_INVALID_ARGUMENT,
 * nothing touched, the capture stays valid, the gaze stays pending): make the call once outside the capture.  A captured graph replays the
 * gaze it was captured with.  A ctx on which no gaze was ever set allocates, uploads and launches exactly what it always has.
 *
 * OVRFSR_ERR_INVALID_ARGUMENT -- the stored value left as it was -- for a NULL ctx, an eye other than OVRFSR_EYE_LEFT / OVRFSR_EYE_RIGHT, or
 * a coordinate that is NaN, infinite or outside [-1, 2]. */
OVRFSR_API int ovrfsr_set_gaze(ovrfsr_ctx *ctx, int eye, float x, float y);
OVRFSR_API int ovrfsr_clear_gaze(ovrfsr_ctx *ctx, int eye);
/* xy: the gaze, or the eye's cfg.proj_centre where none is set (*is_set = 0).  OVRFSR_ERR_INVALID_ARGUMENT for a NULL argument or a bad eye. */
OVRFSR_API int ovrfsr_get_gaze(const ovrfsr_ctx *ctx, int eye, float xy[2], int *is_set);
/* re-aims in place and rebuilds that applies performed because of a gaze, since the ctx was created */
OVRFSR_API int ovrfsr_gaze_stats(const ovrfsr_ctx *ctx, uint32_t *reaims, uint32_t *rebuilds);

/* ---- dynamic resolution: the input size follows the renderer's viewport, per frame -----------------------
 * An engine with dynamic resolution keeps its eye texture at a fixed allocation and renders into a viewport whose size changes from frame to
 * frame; the compositor's target does not move.  Without these calls an input-size change is a full reset: every table and ctx-owned image
 * freed (the output the compositor may still hold included), everything re-planned and uploaded again with blocking copies, the device
 * synchronised by the frees.  With a MAXIMUM input size declared, an apply whose input size differs from the planned one RE-SCALES IN PLACE
 * as long as format, eye layout and output size stay the same.  No ABI version and no config field changes with these: a host probes for
 * the symbols.
 *
 * max_width, max_height: 1..16384 texels per axis, the allocation's size; (0, 0) clears the setting.  Like ovrfsr_set_hidden_area and
 * ovrfsr_set_hdr_domain the setter drops a recorded pair_submit eye, enables a disabled ctx again and makes the next apply plan afresh; it
 * touches no device resource itself, so it is accepted under stream capture.  ovrfsr_reset and ovrfsr_set_config keep the value.
 *
 * THE RULE.  With a maximum set, every call behaves as the same call on a fresh ctx -- same cfg, meshes, gazes and HDR domain, the same
 * maximum set -- that never saw another input size: status, error text, the image handed back, every byte written,
 * ovrfsr_hidden_area_stats; in every form, format, build and precision, for batches, shared side-by-side textures and pair_submit (a texture
 * of another size is still "a recorded eye whose other eye does not follow": the recorded eye is launched first, at its own size).  Only
 * the cost differs, and the address of the ctx-owned output does not move across re-scales.
 *
 * WHAT AN APPLY AFTER AN INPUT-SIZE CHANGE DOES, one of three (ovrfsr_rescale_stats counts the first and the second):
 *   - a RE-SCALE in place: the new size is within the maximum and the plan of the new size differs from the current one in nothing but the
 *     input size, the EASU / NIS constants, the LDS footprints, the bilinear tap tables and the tile records.  No allocation, no blocking
 *     copy, no host wait, nothing freed: the tap tables are refilled and the records rebuilt on the device, on the call's stream; the
 *     launches behind them read the new constants.  Every buffer sized by the input (the multisample resolve's and the R11G11B10F unpack
 *     pass's copy, the BGRA8 re-order's, the HDR domain's mapped copy) was allocated for the maximum when the ctx was built;
 *   - a REBUILD, today's path: the output size moves (cfg.out_width or cfg.out_height is 0), the input now equals the output (no upscale
 *     stage), the form, the tile lists or the outside-tile kernel's stream would change, or the size exceeds the maximum.  Where the plan
 *     of the new size is a refusal (LDS footprint, NVScaler outside 1x..2x) the call fails exactly as on a fresh ctx and the ctx is
 *     disabled until reset;
 *   - nothing: the size is the planned one.
 * A gaze that moved in the same apply is re-aimed behind the re-scale.  Under stream capture an apply that would re-scale or rebuild is
 * refused like any build (OVRFSR_ERR_INVALID_ARGUMENT, nothing touched, the capture stays valid); a captured graph replays the size it was
 * captured with.  Tap clamping happens at the edge of the image the call names: with `data` at the viewport's origin, `width` / `height`
 * the viewport's and `pitch_bytes` the allocation's, no texel of the allocation outside the viewport is ever read.  A ctx on which no
 * maximum was ever set plans, allocates, uploads and launches exactly what it always has.
 *
 * OVRFSR_ERR_INVALID_ARGUMENT -- the stored value left as it was -- for a NULL ctx, one axis zero and the other not, or an axis above 16384. */
OVRFSR_API int ovrfsr_set_max_input_size(ovrfsr_ctx *ctx, uint32_t max_width, uint32_t max_height);
/* the stored maximum, (0, 0) where none is set.  OVRFSR_ERR_INVALID_ARGUMENT for a NULL argument. */
OVRFSR_API int ovrfsr_get_max_input_size(const ovrfsr_ctx *ctx, uint32_t *max_width, uint32_t *max_height);
/* since the ctx was created: the applies that re-scaled in place, and the applies that rebuilt because of an input-size change while a
 * maximum was set */
OVRFSR_API int ovrfsr_rescale_stats(const ovrfsr_ctx *ctx, uint32_t *rescales, uint32_t *rebuilds);

/* ---- mask feather: the edge of the radius mask, ramped over a band -----------------------------------------
 * The radius mask's edge is a staircase of 16x16 groups: EASU + RCAS at full sharpness on one side of a group boundary, a plain bilinear
 * sample on the other.  With a feather WIDTH set, one small pass runs behind the unchanged pipeline, over the band only, and blends every
 * band pixel between what the pipeline stored there and the value that pixel has when its group is outside, by an integer weight that
 * falls from 256 to 0 across the band.  No kernel of the pipeline changes, no plan, no tile list: the pass goes by the mask constants the
 * launches in front of it carried.  No ABI version and no config field changes with these: a host probes for the symbols.
 *
 * width: in cfg.radius's unit (out_height / 2); 0 = off, the default; finite, 0 <= width <= 2.
 *
 * THE RULE.  For one apply, centre[4] and R = radius[0] are what ovrfsr_mask_constants gives that apply, a gaze included.
 *     F   = f2u(0.5f * width * out_height)     the expression of radius[0], the same float -> uint rule
 *     Ro  = R > 12 ? R - 12 : 0                outer edge of the ramp (12: the guard, below)
 *     Ri  = Ro > F ? Ro - F : 0                inner edge
 *     den = Ro * Ro - Ri * Ri                  64-bit
 * The feather is ACTIVE for an eye iff F >= 1, Ro >= 1 and that eye's groups are mixed (some inside, some outside the radius).  For output
 * pixel (x, y), in signed 64-bit integers with the centre words zero-extended:
 *     d2 = min over the two centres k of (cx_k - x)^2 + (cy_k - y)^2
 *     w8 = clamp(floor(256 * (Ro * Ro - d2) / den), 0, 256)
 * A pixel is a BAND PIXEL iff its 16x16 group is inside by the reference's own rule (fsr_easu.hlsl:41-45, uint32 wrap-around and all,
 * unchanged) and w8 < 256.  Pixels of outside groups are never touched.  A band pixel gets, per RGB channel, in fp32 with every operator
 * rounded once and nothing fused,
 *     t = w8 / 256.0f        v = o + (s - o) * t
 * stored with the destination's store conversion; alpha keeps the stored value.
 *   s  the destination's texel as the pipeline stored it, decoded: the byte the same call writes with the feather off.
 *   o  the value that pixel has when its group is OUTSIDE, in the reference's operator order (the strict build's and the oracle's value),
 *      decoded from the destination format: (1) the bilinear fallback sample (D3D rule, unfused); (2) where a sharpen stage follows, stored
 *      to and reloaded from the intermediate format, then the RCAS outside branch's debug_mode tint; (3) stored to and reloaded from the
 *      destination format.
 * THE GUARD of 12 makes every pixel with w8 > 0 lie in an inside group: a pixel is at most sqrt(8^2 + 8^2) = 11.32 from its group's centre,
 * a pixel with w8 > 0 has d < Ro = R - 12, so its group's centre is closer than R to the mask centre.  w8 is therefore 0 everywhere along
 * the staircase: a band pixel there holds exactly o, and the step is gone.  The fully sharp region shrinks to d < Ri; a host compensates
 * with cfg.radius (raise both together).
 *
 * WHERE IT APPLIES.  Every FSR form with an upscale stage (upscale-only, two-pass, mask-sorted, fused, fused with outside tiles), all three
 * precisions (OVRFSR_PRECISION_FP32_EXACT keeps its promise: s is the strict byte, the blend is deterministic), batches, shared
 * side-by-side textures, pair_submit, gaze and re-scale.  Under a hidden-area mesh the pixels of skipped tiles are neither read nor
 * written.  Under OVRFSR_HDR_DOMAIN_SRTM the pass belongs to step 3 of that contract: it runs on the mapped RGBA32F copy and the RGBA32F
 * result, in front of the back pass.  NIS (cfg.use_nis) and the sharpen-only forms IGNORE the setting: nothing is launched, their bytes
 * are unchanged.  With the width 0, or an eye whose groups are not mixed, nothing is launched: plans, launches and bytes are what they
 * are without these calls.
 *
 * LATCHING, like ovrfsr_set_gaze: the setter stores the value and nothing else -- no recorded pair_submit eye dropped, no rebuild, a
 * disabled ctx stays disabled.  The apply that launches reads it; a recorded pair launches with the width in effect at its SECOND call.
 * It is accepted under stream capture, and so is the apply behind it (the pass allocates and uploads nothing); a captured graph replays
 * the width it was captured with.  ovrfsr_reset and ovrfsr_set_config keep the value.
 *
 * OVRFSR_ERR_INVALID_ARGUMENT -- the stored value left as it was -- for a NULL ctx or a width that is NaN, infinite, negative or above 2. */
OVRFSR_API int ovrfsr_set_mask_feather(ovrfsr_ctx *ctx, float width);
OVRFSR_API int ovrfsr_get_mask_feather(const ovrfsr_ctx *ctx, float *width);
/* launches of the feather pass since the ctx was created (one per eye pass of an apply with an active eye) */
OVRFSR_API int ovrfsr_mask_feather_stats(const ovrfsr_ctx *ctx, uint32_t *launches);
/* Constants-only, no GPU: the rule above for a whole out_w x out_h image -- per pixel, row-major, w8 (0..256; 256 everywhere where F = 0 or
 * Ro = 0) and whether its group is inside.  radius_px = radius[0], feather_px = F.  `len`: the element count of each array.
 * OVRFSR_ERR_INVALID_ARGUMENT, nothing written, for a NULL pointer, a size of 0 or above 16384, or len < out_w * out_h. */
OVRFSR_API int ovrfsr_mask_feather_weights(const uint32_t centre[4], uint32_t radius_px, uint32_t feather_px, uint32_t out_w, uint32_t out_h,
                                           uint16_t *w8, uint8_t *inside, size_t len);

/* ---- constants-only entry points (known-answer tests; no GPU needed) ------------------------- */

/* FsrEasuCon (src/fsr/ffx_fsr1.h:156-202); con = con0|con1|con2|con3 */
OVRFSR_API void ovrfsr_easu_con(uint32_t con[16], float in_viewport_w, float in_viewport_h, float in_w,
                                float in_h, float out_w, float out_h);
/* FsrRcasCon (src/fsr/ffx_fsr1.h:662-672); `stops` = 2 - 2*clamp(sharpness,0,1) (PostProcessor.cpp:420-421) */
OVRFSR_API void ovrfsr_rcas_con(uint32_t con[4], float stops);
/* imageCentre / radius of UpscaleConstants and SharpenConstants (PostProcessor.cpp:298-305, 331-335) */
OVRFSR_API void ovrfsr_mask_constants(uint32_t centre[4], uint32_t radius[4], uint32_t out_w, uint32_t out_h,
                                      const float proj_centre[4], float cfg_radius,
                                      int texture_contains_only_one_eye, int eye);
/* NVScalerUpdateConfig / NVSharpenUpdateConfig (src/nis/NIS_Config.h:144-255) as PostProcessor.cpp:308,:433
 * call them; cfg256 receives the 256-byte NISConfig; returns 1/0 like the reference's bool. */
OVRFSR_API int ovrfsr_nis_scaler_config(void *cfg256, float sharpness, uint32_t in_w, uint32_t in_h,
                                        uint32_t out_w, uint32_t out_h);
OVRFSR_API int ovrfsr_nis_sharpen_config(void *cfg256, float sharpness, uint32_t in_w, uint32_t in_h);
/* coef_scale / coef_usm, 64 phases x 8 taps (src/nis/NIS_Config.h:261-393) */
OVRFSR_API const float *ovrfsr_nis_coef_scale(void);
OVRFSR_API const float *ovrfsr_nis_coef_usm(void);

/* ---- data formats either side of the path --------------------------------- */

/* Config::Load (src/postprocess/Config.h:30-63): parse the text of an openvr_mod.cfg (JSON with // comments,
 * src/openvr_mod.cfg) into cfg with the reference's defaulting rules.  On a parse error cfg holds the struct
 * defaults and INVALID_ARGUMENT is returned ("Could not read config file").  Hotkey keys are ignored. */
OVRFSR_API int ovrfsr_config_from_json(const char *text, size_t len, ovrfsr_config *cfg);

/* Stand-in for the F7 capture (PostProcessor.cpp:640-657): dump a device image as a binary PPM. */
OVRFSR_API int ovrfsr_save_ppm(const ovrfsr_image *img, const char *path, void *stream);
/* The capture in the reference's own container: a DDS file (SaveDDSTextureToFile, PostProcessor.cpp:652; DX10 header extension, one mip)
 * holding the texels exactly as they sit in the image -- R8G8B8A8_UNORM, R16G16B16A16_FLOAT, R32G32B32A32_FLOAT, R10G10B10A2_UNORM or
 * B8G8R8A8_UNORM --, rows tightly packed.  (ABI 4) */
OVRFSR_API int ovrfsr_save_dds(const ovrfsr_image *img, const char *path, void *stream);

OVRFSR_API uint32_t ovrfsr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OPENVR_FSR_AMD_H */
