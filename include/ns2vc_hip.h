/* ns2vc_hip.h — C ABI of libns2vc_hip.so, the MI355X (gfx950) denoiser engine.
 *
 * Drop-in boundary for ONE path of adelacvg/NS2VC (branch vc-v2): the latent
 * diffusion denoiser `UNet1DConditionModel.forward` driven by the DPM-Solver++ /
 * UniPC sampling loop.  The reference is pure Python/PyTorch, so there is no
 * reference FFI to mirror; each entry point below names the reference call site
 * (file:line under the reference tree) whose work it replaces.  INTEGRATION.md
 * shows the ctypes binding a maintainer adds on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; the message is
 *     available from ns2vc_last_error() (thread-local, valid until the next call);
 *   - all tensor pointers are DEVICE pointers owned by the caller unless the
 *     parameter is documented as "host or device" (copied with hipMemcpyDefault);
 *   - `stream` is a hipStream_t passed as void*; no call blocks the host except
 *     load/finalize/prepare (setup) and the explicitly synchronous helpers;
 *   - API tensors use the reference's layouts: latent/content (B, C, T) "NCT"
 *     fp32 contiguous, prompt (B, Lp, 256) fp32 contiguous, mask (B, Lp) uint8
 *     (1 = keep), timesteps (B) fp32 (fractional values are legal,
 *     sampler/dpm_solver.py:278);
 *   - a kernel-level call (ns2vc_k_*) reads and writes only the LOGICAL elements of the tensors it is given: rows x width at
 *     the given pitch, from the given pointer.  Bytes between the rows (columns [width, pitch), or in front of a tensor that
 *     is a column slice of wider rows) and bytes in front of / behind a tensor are never written and never influence a
 *     result, whatever they hold (NaN, Inf, another tensor's fp32 bits): rows a tile rounds up to are clamped, bounded by the
 *     buffer descriptor or discarded before they reach a reduction.  `res` may alias `out_f32` element for element (same
 *     pointer, same pitch).  Buffers a call is documented to write (a0 under gnp_x, gnp_raw, stats, rowstats, gnp_sync, the
 *     solver state) are outputs in this sense: their logical region only.  tests/test_kernel_bounds_gpu.py pins this;
 *   - operand-typed source tensors (a0 / a1 / a2, q / k / v, yn, a_op): the caller passes pointers on a 16-byte boundary (a
 *     precondition: the launchers do not check source pointers), and row pitches that are multiples of 16 bytes -- a pitch that
 *     is not is refused by the launcher (non-zero return, nothing launched).
 */
#ifndef NS2VC_HIP_H
#define NS2VC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NS2VC_ABI_VERSION 7
#define NS2VC_MAX_LEVELS 8
#define NS2VC_NCOEF 12 /* floats per row of the solver table, ns2vc_amd/schedule.py:COEF_COLUMNS */

typedef struct ns2vc_unet ns2vc_unet; /* opaque engine handle */

/* Mirrors the ctor kwargs NS2VC passes (model.py:391-400) plus the defaults of
 * unet1d/unet_1d_condition.py:151-203 that shape the network. */
typedef struct ns2vc_unet_cfg {
  int32_t latent_channels;    /* 100: out_channels and the x part of in_channels  */
  int32_t content_channels;   /* 256: in_channels - latent_channels               */
  int32_t n_levels;           /* 4                                                */
  int32_t block_out_channels[NS2VC_MAX_LEVELS]; /* 128,256,384,512                */
  int32_t norm_num_groups;    /* 8                                                */
  int32_t cross_attention_dim;/* 256                                              */
  int32_t heads;              /* 8  (the reference's `attention_head_dim`)        */
  int32_t layers_per_block;   /* 2                                                */
  int32_t pool_heads;         /* 64 (addition_embed_type_num_heads)               */
} ns2vc_unet_cfg;

/* Operand precision = what the MFMAs read (activations as GEMM / attention operands, packed weights).  In every mode the
 * residual stream, GroupNorm / LayerNorm statistics, softmax state, accumulators and the solver state are fp32.
 * Measured end-to-end error of the predicted latent vs the reference fp32 CPU path (tests/test_engine_gpu.py):
 *   F32 1e-6, F16 8e-4 (inside the 1e-3 parity gate: the default 16-bit mode), BF16 6.5e-3 (same speed as F16). */
enum { NS2VC_PREC_F32 = 0,  /* fp32 operands, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32) */
       NS2VC_PREC_BF16 = 1, /* bf16 operands (v_mfma_f32_32x32x16_bf16) */
       NS2VC_PREC_F16 = 2   /* fp16 operands (v_mfma_f32_32x32x16_f16); stores saturate at +-65504 */ };

/* ---- library ----------------------------------------------------------------------- */
int ns2vc_abi_version(void);
/* sizeof(ns2vc_gemm_args) as this library was built: the struct grows at its END within an ABI version (the last field is `lens`), so a binding that
 * mirrors it compares sizes before it passes one */
int ns2vc_sizeof_gemm_args(void);
int ns2vc_sizeof_attn_args(void);                /* the same for the attention arguments, whose last fields are `q_lens, k_lens` */
int ns2vc_sizeof_rowchain_args(void);            /* ... and for the row-chain arguments, whose last field is `lens` */
int ns2vc_sizeof_ffn_args(void);                 /* ... and for the fused feed-forward arguments, whose last field is `lens` */
int ns2vc_sizeof_geglu_args(void);               /* ... and for the token-stationary GEGLU arguments, whose last fields are `T, lens` */
const char* ns2vc_last_error(void);
int ns2vc_device_count(int* out_count);
int ns2vc_set_device(int device);               /* one process per GPU: call with LOCAL_RANK */
int ns2vc_device_name(char* buf, int buflen);
/* ABI v5.  1 when workgroup ids that differ by a multiple of 8 run on one XCD of the current device (the dispatcher's round robin;
 * probed once per device with HW_REG_XCC_ID), 0 when they do not, -1 when the probe could not run.  ns2vc_gemm_args.gnp_sync -- rows
 * exchanged between such workgroups through the L2 they share -- is only FAST where this is 1; the engine's `gn_coop` option
 * defaults to it and cannot be switched on elsewhere.  ABI v6: correctness no longer rests on the probe -- the siblings of a row block
 * count their arrivals per XCC id (HW_REG_XCC_ID) and only trust each other's rows when all of them ran on one XCD; otherwise every
 * workgroup builds all its rows itself (a CU-masked stream, another partition mode), counted in ns2vc_unet_gn_coop_alone.  (The
 * dispatcher's round robin does not start at XCD 0 for every launch -- profiles/r05_placement_probe.txt -- so there is no fixed
 * "XCD of workgroup id i" to rely on, only "ids 8 apart share one".) */
int ns2vc_device_xcd_round_robin(int* out);

/* ---- engine lifetime (replaces UNet1DConditionModel.__init__, unet_1d_condition.py:151-607) */
int ns2vc_unet_create(const ns2vc_unet_cfg* cfg, ns2vc_unet** out);
int ns2vc_unet_destroy(ns2vc_unet* h);

/* One call per state-dict tensor, keyed by the reference's parameter name
 * (load_state_dict, inference/infer_tool.py:24-29; model.py:819-829).  `data` is a
 * host or device pointer to contiguous fp32 of the given shape. */
int ns2vc_unet_load_weight(ns2vc_unet* h, const char* key, const void* data, const int64_t* shape, int ndim);
/* Checks that all tensors arrived, packs them for the chosen precision and uploads. */
int ns2vc_unet_finalize_weights(ns2vc_unet* h, int precision);
int ns2vc_unet_num_missing_weights(ns2vc_unet* h, char* first_missing, int buflen);

/* Plan options, by name; call before ns2vc_unet_prepare (an existing plan / workspace is dropped):
 *   "ln_linear" 1|0  LayerNorm by linearity (default 1) vs explicit normalisation passes
 *   "fold_ff"   1|0  ff.net.2 folded into proj_out at pack time (default 1) vs two launches
 *   "fuse_ffn"  1|0  GEGLU feed-forward + proj_out in ONE launch where eligible (16-bit precisions, dim <= 256; needs
 *                    ln_linear and fold_ff; default 1) vs the GEGLU GEMM + the folded GEMM
 *   "masked_fuse" 1|0  (default 0) a plan built under per-item lengths keeps the fused launches whose kernels mask their own rows
 *                    (ns2vc_gemm_args.lens) instead of the unfused launches described at ns2vc_unet_set_lengths; dense plans ignore it
 *   "masked_attn" 1|0  (default 0) a plan built under per-item lengths gives the attention launches the level's length table (ns2vc_attn_args.q_lens /
 *                    k_lens) instead of the self-attention key-bias row and the mask_rows launch behind each of them; independent of masked_fuse;
 *                    dense plans ignore it.  A plan built under per-item PROMPT lengths (ns2vc_unet_set_prompt_lengths) gives the attn2 launches
 *                    the prompt table as k_lens instead of the bias row (which they keep only where a mask was given): the key tiles past an
 *                    item's prompt are skipped; q_lens as above under latent lengths.  The fp8 PV form and fuse_xattn's in-kernel
 *                    cross-attention keep the bias row
 *   "masked_rows" 1|0  (default 0) a plan built under per-item lengths keeps the two row-chain launches of a transformer block (ns2vc_k_rowchain)
 *                    and gives them the level's length table (ns2vc_rowchain_args.lens) instead of the GroupNorm apply, proj_in, norm1, attn1.qkv,
 *                    attn1.to_out, norm2, attn2.to_q launches and their mask_rows sweeps; independent of masked_fuse and masked_attn; dense plans
 *                    ignore it
 *   "masked_ffn" 1|0  (default 0) a plan built under per-item lengths keeps the pre-stage launch of the fused feed-forward of a dim-128 / 256
 *                    transformer block (ns2vc_k_ffn with pre_a) and gives it the level's length table (ns2vc_ffn_args.lens) instead of the
 *                    attn2.to_out, norm3, ff.geglu, ff.out+proj_out launches and their mask_rows sweeps; independent of masked_fuse, masked_attn
 *                    and masked_rows; dense plans and the fp32 engine ignore it
 *   "attn_resident" 1|0 (default 1) dense fp16 / bf16 attention at head dim 16 / 32 on the K/V-resident kernel (one workgroup per (item, head), the head's
 *                    K/V staged once) where the key rows fit the LDS (<= 1024 / 640 keys) and B * heads >= the device's CUs; 0 = the tiled kernel everywhere.
 *                    Bit-identical results either way.
 *   "masked_geglu" 1|0 (default 0) a plan built under per-item lengths keeps the token-stationary GEGLU launch of a dim-384 transformer block
 *                    (ns2vc_k_geglu) on a level of at least the dense crossover's rows and gives it the level's length table
 *                    (ns2vc_geglu_args.T, lens) with ln_stats = NULL -- the kernel takes the LayerNorm sums from the operand rows it holds --
 *                    instead of the norm3 launch and the plain GEGLU GEMM with its mask_rows sweep; attn2.to_out and ff.out+proj_out stay as
 *                    they are; independent of the four options above; dense plans and the fp32 engine ignore it
 *   "masked_attn_resident" 1|0 (default 0) the attention launches that "masked_attn" has given a length table run on the K/V-resident kernel's masked
 *                    form where "attn_resident" would take them without the table (fp16 / bf16, head dim 16 / 32, the PADDED key rows <= 1024 / 640,
 *                    B * heads >= the device's CUs); bit-identical results, same launches.  Without "masked_attn" and "attn_resident" it does nothing
 * The environment variables NS2VC_LN_LINEAR / NS2VC_FOLD_FF / NS2VC_FUSE_FFN set the defaults at ns2vc_unet_create.
 *   "temb_join_skip" n  (tests, not a plan option) record the fork_temb join at the (n+1)-th reader of the time scale /
 *                    shift rows instead of the first; the plan build then refuses the fork (ns2vc_unet_op_info which = 2) */
int ns2vc_unet_set_option(ns2vc_unet* h, const char* name, int value);
/* LayerNorm-by-linearity health: the largest |mean| / std over every LayerNorm input row seen since the last read-out
 * (or since prepare).  The 16-bit modes round the raw row before centring, so their error on a row grows ~linearly
 * with this ratio (1 at ratio <~ 1; use "ln_linear" 0 when it is >> 10); in fp32 the variance E[x^2] - mean^2 loses
 * ~ratio^2 ulps.  The read-and-reset is enqueued on `stream` (the stream the evaluations ran on), never on the legacy
 * stream:  ns2vc_unet_ln_ratio      = enqueue + synchronise THAT stream + return the value;
 *          ns2vc_unet_ln_ratio_post = enqueue only (no host wait);
 *          ns2vc_unet_ln_ratio_poll = non-blocking: *out_ready = 1 and the value of the last post once it has completed. */
int ns2vc_unet_ln_ratio(ns2vc_unet* h, float* out_ratio, void* stream);
int ns2vc_unet_ln_ratio_post(ns2vc_unet* h, void* stream);
int ns2vc_unet_ln_ratio_poll(ns2vc_unet* h, float* out_ratio, int* out_ready);

/* Allocate workspace and build the launch plan for a (batch, frames, prompt frames) shape. */
int ns2vc_unet_prepare(ns2vc_unet* h, int B, int T, int Lp);
int ns2vc_unet_workspace_bytes(ns2vc_unet* h, size_t* out);

/* Step-invariant work, once per utterance batch: add_embedding(prompt)
 * (unet_1d_condition.py:869-870), the 32 cross-attention to_k/to_v(prompt)
 * (attention_processor.py:1019-1020), the content half of conv_in over cat([x, content])
 * (model.py:409, unet_1d_condition.py:943) and the mask -> bias conversion (:816-818).
 * content (B, content_channels, T); prompt (B, Lp, cross_dim); mask (B, Lp) or NULL. */
int ns2vc_unet_set_condition(ns2vc_unet* h, const float* content_bct, const float* prompt_blc, const uint8_t* mask_bl, void* stream);
/* The two halves of set_condition, for callers whose content and prompt change at different rates (the drop-in
 * nn.Module receives cat([x, content]) anew on every solver step, model.py:409, while the prompt tensor persists):
 * set_content = content half of conv_in only; set_prompt = cross-attention K/V, add_embedding (+ set_mask);
 * set_mask = the (B, Lp) keep-mask -> additive bias conversion only (NULL = no mask), for a mask tensor that is rebuilt
 * per call (model.py:412) over an unchanged prompt. */
int ns2vc_unet_set_content(ns2vc_unet* h, const float* content_bct, void* stream);
int ns2vc_unet_set_prompt(ns2vc_unet* h, const float* prompt_blc, const uint8_t* mask_bl, void* stream);
int ns2vc_unet_set_mask(ns2vc_unet* h, const uint8_t* mask_bl, void* stream);
/* Per-item valid lengths (backward-compatible addition to ABI v7): lengths_b = HOST array [B] with 1 <= L_b <= T, or NULL = dense (every item T
 * frames).  Item b of the padded batch then gives on frames [0, L_b) what the engine gives for that item alone at T = L_b (to the precision's
 * rounding), and exactly 0 on frames >= L_b; per level the valid length is ceil(L / 2) per stride-2 level (ns2vc_amd.spec.level_lengths).  An out-of-range
 * value returns an error and changes nothing; ns2vc_unet_prepare resets to dense.  Call it BEFORE set_condition / set_content for the batch (the
 * content's padded frames are zeroed there).  The first non-NULL call after dense rebuilds the plan as a masked plan (and drops a captured step graph):
 * GroupNorm statistics from their own pass, the fused GroupNorm prologues, row chains, LayerNorm by linearity and fused feed-forward replaced by their
 * unfused launches, the rows past an item's end zeroed after every launch that writes them, the self-attention keys there masked, the nearest upsampling
 * materialised.  Later calls with other lengths only copy the (levels x B) table and the key-mask rows on `stream` (from pinned staging: lengths_b may be reused
 * on return, and the host waits for nothing but the previous call's copy; a repeat of the current lengths copies nothing): a captured graph stays valid. */
int ns2vc_unet_set_lengths(ns2vc_unet* h, const int32_t* lengths_b, void* stream);
/* Per-item prompt lengths (backward-compatible addition to ABI v7): plens_b = HOST array [B] with 1 <= P_b <= Lp, or NULL = dense (every item Lp prompt
 * frames).  Item b of the batch then gives what the engine gives for that item alone with a prompt of P_b frames and no mask (to the precision's
 * rounding), and nothing a prompt row at or past P_b holds (NaN and Inf included) reaches any result.  An out-of-range value returns an error and changes
 * nothing; ns2vc_unet_prepare resets to dense.  Call it BEFORE set_condition / set_prompt for the batch: the engine's prompt copy is zeroed past P_b
 * there, add_embedding's class token is the mean over the item's P_b frames and its attention pooling takes the keys [0, P_b + 1) -- the summation
 * order and bounds of a launch at Lp = P_b, so the item's add_embedding row has that launch's bits wherever the pooling's q|k|v GEMM runs on the same
 * tile -- and attn2 of every block drops the keys at or past P_b: by an additive bias row (the value the mask conversion writes for a dropped key),
 * or, with option masked_attn, by ns2vc_attn_args.k_lens.  The device table lives behind everything the dense plan carves (and behind the tables of
 * ns2vc_unet_set_lengths): the dense layout does not move.  The first non-NULL call after dense rebuilds the (cheap) plan and drops a captured step
 * graph, as ns2vc_unet_set_mask does when a bias appears.  Later calls for the same shape are one copy of the table on `stream` (from pinned staging:
 * plens_b may be reused on return) plus the bias-row launch: a captured graph stays valid; a repeat of the current lengths copies nothing.  With a
 * mask_bl also given the mask applies to the keys below P_b; the pooling ignores the mask, as it does without lengths (the reference's semantics of
 * encoder_attention_mask: unmasked pooling).  Independent of ns2vc_unet_set_lengths: both may be set. */
int ns2vc_unet_set_prompt_lengths(ns2vc_unet* h, const int32_t* plens_b, void* stream);

/* One denoiser evaluation = Diffusion_Encoder.forward (model.py:403-415) ->
 * UNet1DConditionModel.forward (unet_1d_condition.py:743-1037) for the condition set above.
 * x (B, latent_channels, T); t (B) fp32; out (B, latent_channels, T). */
int ns2vc_unet_forward(ns2vc_unet* h, const float* x_bct, const float* t_b, float* out_bct, void* stream);

/* ---- sampling loop (replaces DPM_Solver.sample sampler/dpm_solver.py:1171-1213 and
 * UniPC.sample sampler/uni_pc.py:606-658 incl. the x_start wrapper :271-292/:170-191).
 * `coef` = host array [steps][NS2VC_NCOEF] built by ns2vc_amd.schedule.build_table. */
int ns2vc_sampler_load(ns2vc_unet* h, int steps, const float* coef_host);
/* Per-item schedules (backward-compatible addition to ABI v7): every item of one batch runs its own solver / steps / order inside ONE loop --
 * what took one DPM_Solver.sample / UniPC.sample call (sampler/dpm_solver.py:1171-1213, sampler/uni_pc.py:606-658) per group of requests that
 * agree on every sampler setting.  table_rows = HOST [n_tables] row counts of the distinct tables, coef_host = their rows back to back
 * ([sum(table_rows)][NS2VC_NCOEF], at most 1024 rows together: the device table's fixed capacity); item b of the n_items loop items (the
 * prepared B; n under guidance -- set the guidance first) walks table item_table[b] beginning at loop step item_start[b] >= 0.  The loop runs
 * S = max_b(item_start[b] + rows_b) steps; at loop step r item b is ACTIVE when 0 <= r - item_start[b] < rows_b and uses that row of its table;
 * otherwise it is HELD: its evaluation runs at the clamped row's timestep, its result is ignored and no bit of its solver state changes.  Every
 * item ends on what ns2vc_sampler_load with its table alone gives it, bit for bit; a stochastic item's Philox row word is its local row.  The
 * records go to the device on `stream` from pinned staging: new schedules of the same form replay the captured step graph; switching the form on
 * (this call) or off (ns2vc_sampler_load), and a change of the batch's union of "some item has history 2" / "some item adds noise", recapture.
 * ns2vc_sampler_begin needs seeds when some item adds noise; the x0 correction stays per batch and is refused then; ns2vc_sampler_handoff needs
 * the same tables and records on both engines.  ns2vc_amd.schedule.build_tables / run_tables_numpy are the host statement. */
int ns2vc_sampler_load_items(ns2vc_unet* h, int n_tables, const int32_t* table_rows, const float* coef_host, int n_items, const int32_t* item_table,
                             const int32_t* item_start, void* stream);
/* x (B, latent_channels, T): x_T in, sample out.  use_graph != 0 replays one captured
 * hipGraph per step (no host sync inside the loop). */
int ns2vc_sampler_run(ns2vc_unet* h, float* x_inout_bct, int use_graph, void* stream);
/* The same loop in parts (ns2vc_sampler_run = begin + steps(all) + end), so that a second engine can take over in
 * mid-loop.  Use: MIXED PRECISION -- the last evaluations of a loop dominate the error of the sampled latent (the final
 * second-order update of DPM-Solver++(2M), dpm_solver.py:796-831, extrapolates over a large log-SNR step), so a 16-bit
 * engine runs steps [0, N-k) and an fp32 engine, prepared for the same shape / condition / table, runs the last k:
 *   begin(h16, x_T); steps(h16, N-k); handoff(h32, h16); steps(h32, k); end(h32, x_out).
 * handoff copies the fp32 solver state (x_e, x_bar, d1, m_prev, loop position) on `stream`.
 * Order-3 tables (a nonzero column 10 or 11: d2c, pe) also keep m_{i-2}, in a buffer of the engine allocated by the first begin (or
 * handoff) that needs it, zeroed by begin and copied by handoff; a change between such a table and any other rebuilds the captured step
 * graph, and these tables never run the update in conv_out's epilogue (fuse_solver). */
int ns2vc_sampler_begin(ns2vc_unet* h, const float* x_T_bct, void* stream);
int ns2vc_sampler_steps(ns2vc_unet* h, int n_steps, int use_graph, void* stream);
int ns2vc_sampler_end(ns2vc_unet* h, float* x_out_bct, void* stream);
int ns2vc_sampler_handoff(ns2vc_unet* dst, ns2vc_unet* src, void* stream);   /* both engines must hold the SAME table (compared by hash); the seeds go along */
/* Stochastic samplers (backward-compatible addition to ABI v7): DDPM and DDIM with eta > 0 (ns2vc_amd.schedule.build_table) put a nonzero
 * noise coefficient in column 9 of a table row; the update then adds noise * z, z drawn on the device by Philox4x32-10 keyed by the item's
 * seed with counter (t, c / 4, step, 0) (ns2vc_amd/noise.py states the stream), on frames t < L_b and channels c < latent_channels only.
 * A row whose coefficient is 0 adds nothing, so noise-free tables keep their bits.  seeds_b = HOST array [B] of 64-bit seeds, copied on
 * `stream` from pinned staging (a captured step graph stays valid; seeds_b may be reused on return).  ns2vc_unet_prepare clears them, and
 * ns2vc_sampler_begin refuses a stochastic table without them.  Stochastic tables never run the update in conv_out's epilogue (fuse_solver). */
int ns2vc_sampler_set_seeds(ns2vc_unet* h, const uint64_t* seeds_b, void* stream);
/* Classifier-free guidance (backward-compatible addition to ABI v7; replaces model_wrapper's guidance_type="classifier-free", condition,
 * unconditional_condition, guidance_scale: sampler/uni_pc.py:155-233, sampler/dpm_solver.py:170-333).  The engine is prepared for B = 2n items and
 * given the condition cat([unconditional, conditional]) -- rows [0, n) unconditional, [n, 2n) conditional, as the reference batches them
 * (uni_pc.py:222-229) -- and, where it runs per-item lengths, `lengths` and `prompt_lengths` of 2n entries; the two halves MUST hold the same
 * latent lengths (ns2vc_sampler_begin refuses otherwise).  scale_host = HOST array [n] of finite per-item scales, copied on `stream` from pinned
 * staging as the seeds are: later calls with new values replay the captured step graph.  scale_host = NULL turns guidance off.  A change of
 * on / off drops the step graph, clears the seeds and ends a loop in progress; ns2vc_unet_prepare turns guidance off.
 * With guidance on, ns2vc_sampler_begin / _run / _peek / _end take and give n items, ns2vc_sampler_set_seeds takes n seeds (both halves get the
 * same noise) and every step combines x0_g = x0_u + scale[b] * (x0_c - x0_u) in front of the unchanged update (the reference combines in noise
 * space; eps is affine in x0 with the same x, alpha, sigma in both halves, so it is the same point).  scale[b] == 1 takes x0_c itself: such an
 * item follows its unguided trajectory.  The update never runs in conv_out's epilogue (fuse_solver is ignored).  ns2vc_sampler_handoff carries
 * the guidance of `src` (on / off, n, the scales) over to `dst`. */
int ns2vc_sampler_set_guidance(ns2vc_unet* h, const float* scale_host, int n, void* stream);
/* Correction of the predicted x0 inside the loop (backward-compatible addition to ABI v7; the constructor options correcting_x0_fn,
 * thresholding_max_val, dynamic_thresholding_ratio of the reference's two continuous solvers: sampler/dpm_solver.py:338-425, :433-442,
 * sampler/uni_pc.py:236-294).  mode 0 = off; 1 = "dynamic_thresholding": per item and step s_b = max(quantile_ratio(|m_b|), max_val), then
 * m_b = clamp(m_b, -s_b, s_b) / s_b, with m the model value after the x_start round trip (the guided one under guidance) and the quantile
 * torch.quantile's (linear interpolation in float32) over the item's own elements -- frames t < L_b, channels c < latent_channels; 2 = clamp(m,
 * -max_val, max_val), the common callable.  The corrected m is what enters the update and the histories.  The quantile is an exact selection on the
 * device (one launch per step in front of the update), so the loop still captures.  0 <= ratio <= 1, max_val finite and > 0.  A change of mode, or
 * of a value the active mode passes to its launches (mode 1: ratio and max_val; mode 2: max_val), drops the captured step graph; a repeat of the
 * same values, or a change of a value no launch takes (the ratio under mode 2, either while off), does not.
 * ns2vc_sampler_begin / _steps refuse a correction together with a stochastic table (the reference's ddim_sample / p_sample_loop have none), the
 * update never runs in conv_out's epilogue under a correction (fuse_solver is ignored), ns2vc_unet_prepare leaves the setting alone, and
 * ns2vc_sampler_handoff carries that of `src` over to `dst`. */
int ns2vc_sampler_set_x0_correction(ns2vc_unet* h, int mode, float ratio, float max_val);
/* The correction as a per-item table (backward-compatible addition to ABI v7): loop item b is corrected by its own record
 * (mode_host[b], ratio_host[b], max_val_host[b]) -- HOST arrays [n], n = the loop items (n, not 2n, under guidance), every record under the rules
 * above (mode 0 .. 2, 0 <= ratio <= 1, max_val finite and > 0, also where the mode does not read them).  The records live in device memory and
 * are copied on `stream` from pinned staging as the seeds and the scales are: new values replay the captured step graph.  All three pointers
 * NULL = off.  What recaptures: switching the table on or off, a larger record buffer, and -- outside slot mode -- the first record in mode 1 or
 * the last one gone (the quantile launch is issued only when a record needs it; a slot loop always issues it).  Item b ends on the bits it has
 * when the same loop runs with ns2vc_sampler_set_x0_correction(mode_b, ratio_b, max_val_b); a held or idle item is not touched and its
 * threshold is not written.
 * The table and the loop-wide setting exclude each other: this call is refused while ns2vc_sampler_set_x0_correction has a mode != 0, and
 * ns2vc_sampler_set_x0_correction(mode != 0) is refused while the table is on.  The table reads per-item records: ns2vc_sampler_begin on a
 * shared table (ns2vc_sampler_load) is refused with the table on -- use ns2vc_sampler_load_items or a slot loop.  A stochastic item (ddim with
 * eta > 0, ddpm) has no correction: a record with mode != 0 on an item whose table has a noise column is refused by
 * ns2vc_sampler_load_items, ns2vc_sampler_begin and ns2vc_sampler_admit (and by this call for the busy slots of a slot loop), per item -- corrected and stochastic items may share a loop.
 * Slot mode: ns2vc_sampler_open bakes in whether the table is on (set it, all modes 0, before opening) and allocates the thresholds; in
 * mid-loop the call is a whole-vector copy under the rule for seeds and scales: change the entries of idle slots only.
 * fuse_solver is ignored under the table, ns2vc_unet_prepare leaves it alone, ns2vc_sampler_handoff carries it over to `dst`. */
int ns2vc_sampler_set_x0_correction_items(ns2vc_unet* h, const int32_t* mode_host, const float* ratio_host, const float* max_val_host, int n, void* stream);
/* Known frames (backward-compatible addition to ABI v7): per loop item b a set of frames K_b whose predicted x0 is a latent the
 * caller supplies -- the fixed context of a chunked long utterance, or the part of an utterance that a partial re-synthesis keeps.  known_nct =
 * DEVICE [n][latent_channels][T] fp32 (the whole tensor is read, on `stream`, into the engine's own rows; values off the mask are ignored), mask_nt = HOST [n][T] uint8 (nonzero = held), n = the loop items (n,
 * not 2n, under guidance: set the guidance first).  At every evaluation, between the plan's last launch and the solver update, ONE launch writes
 * x0[b, t, c] = known[b, c, t] for t in K_b and c < latent_channels and 0 for the pad columns of those rows, in both halves of a guided engine
 * (the guided combination of two equal values is that value at every scale); every other row of x0 keeps every bit.  The update itself is
 * unchanged and runs in fp32 on the fp32 x0 in every precision.  Every solver here is linear in the model value, so a held frame follows the
 * forward marginal x_i = alpha_i k + sigma_i eps with the one eps of its start state; the caller forms x_T = alpha_0 k + sigma_0 noise there
 * (ns2vc_amd.schedule.known_start).  The launch is sized by the held rows: their list and its count live in device memory beside the known rows,
 * in buffers for the whole prepared shape, copied on `stream` from pinned staging -- new values and new masks replay the captured step graph,
 * switching the hold on or off drops it.  NULL, NULL = off.  Refused: n other than the loop items; a held frame at or past the item's length
 * (ns2vc_unet_set_lengths; set the lengths first, ns2vc_sampler_begin checks again); an x0 correction being on, in either form -- it would
 * rescale the held frames -- and, the other way round, ns2vc_sampler_set_x0_correction (mode != 0) and ns2vc_sampler_set_x0_correction_items
 * while a hold is on; a slot loop, and ns2vc_sampler_open while a hold is on.  ns2vc_sampler_handoff refuses two engines that disagree on
 * whether a hold is set: set it on both.  The update never runs in conv_out's epilogue under a hold (fuse_solver is ignored);
 * ns2vc_unet_prepare and a change of guidance on / off switch the hold off. */
int ns2vc_sampler_set_known(ns2vc_unet* h, const float* known_nct, const uint8_t* mask_nt, int n, void* stream);
/* x_e of a loop in progress (the point the next evaluation is taken at) without ending the loop: what a precision self-check
 * evaluates two engines on (ns2vc_amd.pipeline.Denoiser) */
int ns2vc_sampler_peek(ns2vc_unet* h, float* x_out_bct, void* stream);
/* workgroups of the attention launches of this engine whose optimistic pass (no per-tile maximum; r3) had to be repeated by the
 * exact pass since the last reset -- each of them paid the kernel twice.  Synchronises `stream`. */
int ns2vc_unet_attn_fallbacks(ns2vc_unet* h, unsigned long long* count, int reset, void* stream);
/* ABI v5.  Workgroups of the cooperative GroupNorm prologue (ns2vc_gemm_args.gnp_sync, option `gn_coop`) that waited in vain for a
 * sibling since the plan was built (or the last reset) and built all their rows themselves: a performance counter -- the results do
 * not depend on it.  Synchronises `stream`. */
int ns2vc_unet_gn_coop_alone(ns2vc_unet* h, unsigned long long* count, int reset, void* stream);
/* Backward-compatible addition to ABI v7.  Step graphs this engine has captured and instantiated since it was created: a captured loop that finds its
 * graph still valid replays it and leaves the count alone (new lengths, prompt lengths, seeds or a new condition for the same shape); whatever drops
 * the graph (prepare, an option, the first lengths / prompt lengths / mask after none, another kind of solver table) makes the next captured loop
 * count one more.  No device work, no wait. */
int ns2vc_unet_graph_captures(ns2vc_unet* h, unsigned long long* count);

/* ---- introspection for tests / profiling -------------------------------------------- */
int ns2vc_unet_set_debug(ns2vc_unet* h, int enable);  /* keep a copy of every block output; drops the plan: call before prepare() */
int ns2vc_unet_num_taps(ns2vc_unet* h);
int ns2vc_unet_tap_info(ns2vc_unet* h, int idx, char* name, int buflen, int* rows, int* cols);
int ns2vc_unet_tap_read(ns2vc_unet* h, int idx, float* host_dst);   /* synchronous, [rows][cols] channels-last */
int ns2vc_unet_num_launches(ns2vc_unet* h, int* per_forward, int* per_condition);
/* which: 0 = per-step forward plan, 1 = condition plan.  kind: 0 other, 1 implicit GEMM, 2 attention,
 * 3 norm statistics, 4 copy.  flops / bytes: algorithmic work of that launch.
 * which = 2: the timestep-embedding branch of the per-step plan (option fork_temb), idx 0..5 -> name = "begin" (its first launch),
 * "end" (one past its last), "join" (the launch a captured step joins it in front of), "first_reader" (the first launch that reads
 * its scale / shift rows), "readers" (how many do), "forks" (1 if a captured step forks the branch), value in *kind.  The plan
 * build refuses the fork ("forks" 0) unless first_reader >= join. */
int ns2vc_unet_op_info(ns2vc_unet* h, int which, int idx, char* name, int buflen, int* kind, double* flops, double* bytes);
/* Per-launch timing of the per-step plan: each launch repeated `reps` times between one hipEvent pair on
 * `stream`; ms[i] = average milliseconds of launch i (n_ms >= launches). Leaves garbage in the workspace. Synchronous. */
int ns2vc_unet_profile_forward(ns2vc_unet* h, float* ms, int n_ms, int reps, void* stream);

/* ---- raw device helpers so tests/bench can drive the ABI without torch ------------------ */
int ns2vc_dev_malloc(void** out, size_t bytes);
int ns2vc_dev_free(void* p);
int ns2vc_memcpy_h2d(void* dst, const void* src, size_t bytes);
int ns2vc_memcpy_d2h(void* dst, const void* src, size_t bytes);
int ns2vc_dev_sync(void);
int ns2vc_stream_create(void** out);
int ns2vc_stream_destroy(void* stream);
int ns2vc_stream_sync(void* stream);
/* ABI v6: a stream whose kernels only run on the CUs whose bit is set (hipExtStreamCreateWithCUMask: bit i % 32 of word i / 32 = CU i of the
 * device's enumeration, XCD-interleaved on MI355X).  For partitioning the chip between the denoiser and the PyTorch stages of a pipeline
 * (ns2vc_amd/pipeline.py) and for the placement tests of the cooperative GroupNorm prologue. */
int ns2vc_stream_create_cu_mask(void** out, const uint32_t* mask_words, int n_words);
int ns2vc_event_create(void** out);
int ns2vc_event_destroy(void* ev);
int ns2vc_event_record(void* ev, void* stream);
int ns2vc_event_elapsed_ms(void* start, void* stop, float* ms);  /* synchronises on `stop` */

/* ---- kernel-level entry points (unit-tested one by one through this ABI) -------------- */
typedef struct ns2vc_gemm_args {  /* implicit GEMM: conv1d k3/k1 (stride 1, stride 2, nearest-up), linear */
  /* "operand" tensors are stored in the engine's MFMA operand type: fp32 (precision 0), bf16 (1) or fp16 (2) */
  const void* a0; const void* a1; /* channels-last operand-typed sources; a1 = second half of a no-copy concat or NULL */
  int32_t lda0, lda1, c0, c1;
  int32_t B, Tin, Tout, M;        /* M = B*Tout output rows */
  int32_t taps, tmode;            /* taps 1|3; tmode 0 same, 1 stride-2, 2 nearest-upsample-then-conv */
  const void* w; int32_t K;       /* packed weights [N][K] from ns2vc_pack_weight */
  int32_t N;
  const float* bias;
  const float* res; int32_t ldres;/* fp32 residual added in the epilogue, or NULL */
  int32_t geglu;
  float* out_f32; int32_t ldo_f32;/* fp32 result (residual stream), or NULL */
  void* out_op; int32_t ldo_op;   /* operand-typed copy of the result (feeds the next GEMM / attention), or NULL */
  /* optional GroupNorm statistics of the result, accumulated by the epilogue: int64 fixed point
   * [B][N/16][2] = (sum * 2^28, sum of squares * 2^16) per batch item and 16-channel block; must be zeroed
   * by the caller; needs Tout >= 64 (a wave's rows then touch at most two batch items), geglu == 0, N % 16 == 0: refused otherwise */
  long long* stats;
  /* optional second K segment (a fused 1x1 conv on another operand tensor, e.g. the resnet shortcut):
   * K = taps*(c0+c1) + c2, out += A2[m, :] * W[:, taps*(c0+c1):]; same row mapping, centre tap */
  const void* a2; int32_t lda2, c2;
  /* LayerNorm by linearity (attention.py:83,102,118 without a normalisation pass):
   *   producer: rowstats != NULL -> the epilogue stores (sum, sum of squares) of every RESULT row per 64-column slice:
   *             fp32 [M][N/64][2], one writer per slot (nothing to zero; geglu == 0, N % 128 == 0);
   *   consumer: ln_stats != NULL -> the A rows are the RAW x of LayerNorm(x) (gamma/beta folded into w/bias) and the
   *             epilogue applies  out = rstd[m] * (acc[m][n] - mean[m] * ln_wsum[n]) + bias[n]  with mean/rstd over
   *             ln_dim channels (128..512, multiple of 128) from the producer's [M][ln_dim/64][2] pairs; ln_wsum[n] = sum_k w[n][k]
   *             of the packed, rounded weights (ns2vc_weight_rowsum). */
  float* rowstats;
  const float* ln_stats; const float* ln_wsum; float ln_eps; int32_t ln_dim;
  unsigned* ln_health;            /* optional (consumer): atomicMax of the bits of |mean| * rstd over the rows, or NULL */
  /* optional GroupNorm-apply prologue (ABI v4; replaces a separate ns2vc_k_groupnorm launch in front of this GEMM, the
   * `group_norm` (+ time scale/shift) (+ SiLU) of resnet.py:606-629 / transformer_1d.py:268): when gnp_x != NULL every
   * workgroup FIRST writes act(GroupNorm(gnp_x)) for exactly the rows its tile will read (its output rows, plus one row
   * either side for taps == 3) into a0 -- same arithmetic as ns2vc_k_groupnorm, bit-identical rows -- and then runs as
   * usual, reading them back through its own L2.  a0 must be writable; c1 == 0, tmode == 0, Tin == Tout, N % 128 == 0,
   * c0 <= 1024, (c0 / gnp_G) % 16 == 0, gnp_G <= 8, Tin >= 66.  gnp_x fp32 [B*Tin][gnp_ldx]; gnp_stats = int64
   * [B][c0/16][2] as left by a producer's `stats`; gnp_gamma / gnp_beta [c0]; gnp_temb (or NULL) points at row 0 of the
   * per-item (scale | shift) pairs: scale at [b*gnp_ldtemb + c], shift at [b*gnp_ldtemb + c0 + c]. */
  const float* gnp_x; int32_t gnp_ldx;
  const long long* gnp_stats; const float* gnp_gamma; const float* gnp_beta;
  const float* gnp_temb; int32_t gnp_ldtemb;
  float gnp_eps; int32_t gnp_G, gnp_silu;
  /* ABI v5 / v6, optional: [ceil(M / 64)] 64-bit arrival words (8-byte aligned), owned by this call site and ZERO when a launch starts (the
   * engine keeps them in the statistics pool, cleared at the start of every forward).  With them (and 2 .. 15 column tiles) the column tiles
   * of a row block -- dispatched as neighbours on one XCD -- build a share of the block's rows each and wait for the others' (bounded),
   * instead of each building all of them.  Same values either way.  ABI v6: the placement is checked, not assumed -- an arrival adds 1 to
   * bits 0-15 and 1 to the 4-bit count of ITS XCC id (bits 16 + 4 * HW_REG_XCC_ID ..), and a workgroup uses its siblings' rows only when
   * all arrivals it sees carry its own XCC id; otherwise (and when it waits in vain) it builds every row itself (gnp_alone).  Bit 62 set:
   * "do not wait" (tests).  Needs a0 128-byte aligned and whole 128-byte lines per row (lda0 * operand size % 128 == 0). */
  unsigned* gnp_sync;
  unsigned* gnp_alone;            /* optional: += 1 per workgroup that waited in vain and built every row itself */
  /* ABI v5, optional: the normalised input is the channel concat of TWO tensors (resnet.py:591 on torch.cat([h, skip]) in the up
   * blocks): the last gnp_c1 of the c0 channels come from gnp_x1 (fp32 [B*Tin][gnp_ldx1], statistics gnp_stats1 [B][gnp_c1/16][2]),
   * the first c0 - gnp_c1 from gnp_x / gnp_stats; gamma / beta / temb index the concatenated channels; groups may straddle the
   * two.  c0 <= 1024, gnp_c1 % 16 == 0.  gnp_raw (or NULL): the un-normalised rows in the operand type, same layout as a0 --
   * the copy a 1x1 shortcut conv reads later. */
  const float* gnp_x1; int32_t gnp_ldx1, gnp_c1;
  const long long* gnp_stats1;
  void* gnp_raw;
  /* ABI v6: kernel choice.  0 = automatic (k = 3 / stride-1 convolutions with Tin >= 66 run on the tap-sharing kernel, convts.hip: the
   * activation chunk of the three taps is loaded once; same result to fp32 rounding, another summation order over K), 1 = never that kernel. */
  int32_t algo;
  /* ABI v6, optional (k = 3 / stride-1 launches only): the same weights as `w` in the tile-major layout of ns2vc_pack_conv3_tiled.  The
   * tap-sharing kernel then reads every (64-column group, step) weight block as 8 KB of consecutive bytes instead of 64 row segments
   * K * 2 bytes apart (-1.1 % of the step: the tiles come from beyond L2 every step); `w` is still required (other kernels, fallbacks). */
  const void* w_tiled;
  /* ABI v7.  algo also takes 2: the tap-sharing kernel with the materialising GroupNorm prologue; with algo = 0 and gnp_x set it MAY normalise
   * inside its K loop instead (nothing is written to a0 then; same values).
   * ABI v7, optional (k = 3 / stride-1 launches of the tap-sharing kernel with ONE column tile, i.e. N == 128: the denoiser's conv_out): the
   * solver update of the sampling loop (sampler/uni_pc.py:471-588, sampler/dpm_solver.py:433-442, 547-580 as restated in
   * ns2vc_amd/schedule.py) applied to the result in the epilogue instead of by a separate ns2vc_k_solver_update launch: with x0 = the
   * conv's result (bias added), row *sol_step of the coefficient table sol_coef [steps][sol_ncoef] and the solver state
   * (sol_xe, sol_xbar, sol_d1, sol_mprev: fp32 [M][sol_ld], updated in place; sol_xe_op: the operand-typed copy of xe the next
   * evaluation's conv_in reads) exactly the arithmetic of ns2vc_k_solver_update, element for element.  out_f32 / out_op may be NULL. */
  const float* sol_coef; const int32_t* sol_step; int32_t sol_ncoef;
  float* sol_xe; void* sol_xe_op; float* sol_xbar; float* sol_d1; float* sol_mprev; int32_t sol_ld;
  /* ABI v7: column tile of the tap-sharing kernel for this launch: 0 = the library's heuristic for the current device, 64 | 128 = fixed.  The engine
   * decides per plan (from ITS device's CU count) and passes the choice along, so that two engines on different devices -- or a debug hook called
   * between plan build and launch -- cannot change a launch's tiling relative to what its plan assumed. */
  int32_t conv_bn;
  /* ABI v7, 16-bit precisions: hi + lo operand pairs (x = hi(x) + lo(x) with hi = the operand type's rounding of x, lo = the rounding of the rest).  A GEMM
   * over [hi | lo | hi] activation columns against [hi(w) | hi(w) | lo(w)] weight columns (the caller packs them so) gives x * w to ~2^-21 relative instead of
   * 2^-11 for 3x the K -- the engine's `split_io` option uses it for conv_in and conv_out (23 % of the fp16 forward error's energy, profiles/r06_error_budget.txt).
   *   gnp_pair = 1: the GroupNorm prologue normalises c0 / 2 channels and writes the pair: hi at a0[r][c], lo at a0[r][c0 / 2 + c]; the launch may then
   *                  carry a1 = a0, c1 = c0 / 2 (the hi plane once more) -- the one case where c1 != 0 goes with gnp_x.  Tap-sharing kernel with the materialising
   *                  prologue only (its own instantiation; other kernels refuse the flag).  Without gnp_x a pair is just a wider operand tensor: any kernel takes it.
   *   sol_op_pair = 1: sol_xe_op rows hold such a pair, [hi(sol_ld) | lo(sol_ld)], row stride 2 * sol_ld (what ns2vc_k_solver_update writes for the engine). */
  int32_t gnp_pair, sol_op_pair;
  /* Per-item valid lengths (backward-compatible addition to ABI v7: the field is the LAST of the struct, NULL = everything above as it was).
   * lens = DEVICE [B], 1 <= lens[b] <= Tout: the kernel keeps the row invariant of a length-masked batch itself.  An output row (b, t) with
   * t >= lens[b] is stored as exact zeros in out_f32 and out_op (bias and residual not added, whatever the accumulator, the residual row or the
   * operand rows behind it hold) and adds nothing to `stats`; with gnp_x the prologue takes mean / rstd over lens[b] * (channels per group)
   * elements instead of Tin * ..., and writes the operand rows (a0, gnp_raw, both planes of a gnp_pair) past lens[b] as zeros.  The per-item
   * period of the rows is Tout (= Tin wherever a prologue runs).  Served by the masked instantiations of the tap-sharing conv kernel (materialising
   * prologue; algo 0 is run as algo 2) and of the 8-wave GEMM kernel without a prologue; every other combination is refused, never run unmasked:
   * rowstats, ln_stats, sol_coef, gnp_x outside the tap-sharing kernel, N % 128 != 0 or a narrow GEGLU (N < 2048) outside it.
   * The struct is 8 bytes longer than in earlier builds of ABI v7 and ns2vc_k_gemm reads all of it: a binding compiled against the earlier header
   * MUST be rebuilt (or it passes 8 bytes of its own memory as `lens`); ns2vc_sizeof_gemm_args() is there to check. */
  const int32_t* lens;
} ns2vc_gemm_args;

typedef struct ns2vc_attn_args {
  const void* q; const void* k; const void* v; /* operand-typed rows; head h lives at columns [h*hd, (h+1)*hd) */
  int32_t ldq, ldk, ldv;
  int32_t B, H, Lq, Lk;
  const float* bias;              /* additive [B][Lk] or NULL */
  float scale;
  void* out; int32_t ldo;         /* operand-typed */
  int32_t pv_fp8;                 /* 16-bit precisions only: 1 = the PV product on the fp8 MFMA (V and the probabilities rounded to OCP e4m3) */
  int32_t exact_only;             /* 1 = skip the optimistic pass (no per-tile maximum) and take the exact pass directly */
  unsigned* fallbacks;            /* device counter or NULL: += 1 per workgroup whose optimistic pass had to be repeated exactly */
  /* Per-item query and key counts (backward-compatible addition to ABI v7: the two fields are the LAST of the struct, both NULL = everything above as
   * it was; either may be NULL on its own).  The row stride between items stays Lq / Lk.
   *   k_lens = DEVICE [B], 1 <= k_lens[b] <= Lk: item b attends to its keys [0, k_lens[b]) only, exactly as the launch does for that item alone at
   *            Lk = k_lens[b] (the same tiles in the same order: its rows are bit-identical to that launch's).  Key and value rows at or past
   *            k_lens[b] are never read; `bias`, when also given, applies to the keys below k_lens[b].
   *   q_lens = DEVICE [B], 1 <= q_lens[b] <= Lq: the rows of `out` at or past q_lens[b] are stored as exact zeros, whatever q holds there (those q
   *            rows are never read).  A 128-query tile wholly past q_lens[b] stores its zeros and returns: no K / V tile staged, no MFMA.  Padded
   *            rows take no part in the optimistic pass's repeat decision and never raise `fallbacks`.
   * Served by the masked instantiations of the attention kernel: every operand type, head width and key tile, optimistic and exact pass.  With
   * pv_fp8 the call is refused (hipErrorInvalidValue), never run unmasked.  The kernel clamps a count to its range before it uses it, so a bad table
   * cannot send a fetch or a store outside the tensors; ns2vc_k_attention also reads the tables back (it waits for `stream`) and refuses a
   * count outside its range before anything is launched.
   * The struct is 16 bytes longer than in earlier builds of ABI v7 and ns2vc_k_attention reads all of it: a binding compiled against the earlier
   * header MUST be rebuilt; ns2vc_sizeof_attn_args() is there to check. */
  const int32_t* q_lens;
  const int32_t* k_lens;
} ns2vc_attn_args;

/* Fused feed-forward + proj_out of one transformer block (attention.py:178-203 GEGLU feed-forward, transformer_1d.py:287-295),
 * 16-bit precisions, dim 128 | 256, T >= 64:
 *   out = [Wpo W2 | Wpo] [GEGLU(LayerNorm(y) W1^T + b1) | y] + (Wpo b2 + bpo) + res
 * `yn` = the RAW rows y in the operand type with their LayerNorm-by-linearity statistics `ln_stats` (as a producer GEMM's
 * `rowstats` leaves them); `wstream` from ns2vc_pack_ffn; `consts` [8*dim][2] = (sum_k of the rounded packed W1 row, folded
 * bias) in packed row order (per 32 hidden units: 32 value rows, then their 32 gate rows); `bias2` [dim]. */
typedef struct ns2vc_ffn_args {
  const void* yn; int32_t ldy;
  const float* ln_stats; float ln_eps;
  const void* wstream; const float* consts; const float* bias2;
  const float* res; int32_t ldres;          /* fp32 block residual x */
  float* out_f32; int32_t ldo_f32;          /* fp32 result, or NULL */
  void* out_op; int32_t ldo_op;             /* operand-typed copy, or NULL */
  long long* stats;                         /* optional GroupNorm statistics of the result, as in ns2vc_gemm_args */
  int32_t B, T, M, dim;                     /* M = B*T rows */
  unsigned* ln_health;                      /* optional, as in ns2vc_gemm_args */
  /* optional pre-stage (attn2.to_out + residual, attention_processor.py:1040-1050): y = pre_a Wo^T + pre_bias + pre_res is
   * computed inside the kernel and never stored; yn / ln_stats are ignored.  wstream must then come from ns2vc_pack_ffn_pre. */
  const void* pre_a; int32_t pre_lda;       /* attention output rows, operand-typed [M][pre_lda] */
  const float* pre_bias;                    /* [dim] */
  const float* pre_res; int32_t pre_ldres;  /* fp32 residual stream before the attention [M][pre_ldres] */
  /* ABI v7, optional, with the pre-stage only: the prompt cross-attention itself (F.scaled_dot_product_attention of attn2,
   * attention_processor.py:1032 with the mask bias of unet_1d_condition.py:816-818) computed INSIDE the kernel for the workgroup's 64 tokens -- the
   * k | v of the prompt are hoisted per utterance, so attn2's SDPA is token-local work: one wave per head (8 heads), two passes over the Lk keys (row
   * maximum, then exp2 / P V with the probabilities rounded to the operand type), the result written straight into the token panel; pre_a is ignored
   * and no attention-output tensor exists.  att_q = attn2.to_q rows [M][att_ldq]; att_kv = ns2vc_k_xattn_pack's image of this layer's k | v rows (MFMA
   * fragments in consumption order: every load of the kernel is 1 KB of consecutive bytes per wave); att_bias = additive mask bias [B][att_Lk] or NULL;
   * att_scale = 1/sqrt(dim/8).  Token blocks are then cut per batch item (ceil(T / 64) workgroups per item). */
  const void* att_q; int32_t att_ldq;
  const void* att_kv; const float* att_bias; float att_scale; int32_t att_Lk;
  /* Per-item frame counts (backward-compatible addition to ABI v7: the LAST field of the struct, NULL = everything above as it was).
   *   lens = DEVICE [B], 1 <= lens[b] <= T, one count per batch item.  Row m is frame t = m - b T of item b = m / T and takes part iff t < lens[b];
   *          a count is clamped to 0 .. T before it is used.
   * A row at or past its item's end: out_f32 and out_op are stored as exact zeros (no bias2, no residual), whatever yn / pre_a hold there; its
   * `res`, `pre_res` and `ln_stats` rows are not read; it takes no part in ln_health and adds nothing to `stats`, which hold the sums over every
   * item's valid rows only.  Every other row is bit-identical to the launch on its item alone at T = M = lens[b].  A 64-row block without a valid
   * row stores its zeros and returns: no weight is streamed for it.  Served by the masked instantiations of the kernel: both operand types, dim 128
   * and 256, the plain and the pre-stage form.  A call that sets `lens` together with att_q (the in-kernel cross-attention has no masked form) or
   * with M != B T is refused (hipErrorInvalidValue), never run unmasked.
   * The struct is 8 bytes longer than in earlier builds of ABI v7 and ns2vc_k_ffn reads all of it: a binding compiled against the earlier header
   * MUST be rebuilt; ns2vc_sizeof_ffn_args() is there to check. */
  const int32_t* lens;
} ns2vc_ffn_args;
/* w1_packed [8*dim][dim]: LayerNorm-folded ff.net.0 rows in the packed (32 value | 32 gate) order; w2f [dim][5*dim] =
 * [Wpo W2 | Wpo]; both fp32 host, row-major.  Returns the device tile stream the kernel consumes. */
int ns2vc_pack_ffn(const float* w1_packed_host, const float* w2f_host, int dim, int precision, void** out_stream_dev);
/* the same with the pre-stage matrix w0 [dim][dim] (attn2.to_out) in front */
int ns2vc_pack_ffn_pre(const float* w1_packed_host, const float* w2f_host, const float* w0_host, int dim, int precision, void** out_stream_dev);
int ns2vc_k_ffn(const ns2vc_ffn_args* a, int precision, void* stream);
/* ABI v7: the k | v image ns2vc_ffn_args.att_kv reads.  k, v = operand-typed rows [B*Lk][ldk / ldv] (head h at columns h*hd ..), 8 heads, hd = 16 | 32.
 * out, per (batch item, head, tile of 32 keys): hd/16 K fragments and 2 V^T fragments of 1 KB each (lane l of a wave reads bytes 16 l ..): K fragment s, lane
 * (key = l % 32, half = l / 32) = k[key][16 s + 8 half .. + 7]; V^T fragment j, lane (d = l % 32, half) = the values v[key(slot)][d] of slots 16 j + 8 half .. + 7,
 * where inside every group of 16 slots key bits 2 and 3 are swapped (the order in which the score MFMA leaves a lane's probabilities); hd 16: row d = 16 is
 * all ones (the softmax denominator rides the P V product), rows above zero; keys beyond Lk zero.  ns2vc_xattn_pack_bytes = size of `out`. */
size_t ns2vc_xattn_pack_bytes(int B, int Lk, int hd);
int ns2vc_k_xattn_pack(const void* k, int ldk, const void* v, int ldv, int B, int Lk, int hd, void* out, int precision, void* stream);

/* r5: token-stationary GEGLU projection (csrc/geglu.hip; 16-bit precisions, dim 384): h = (n W1v^T + b1v) * gelu(n W1g^T + b1g),
 * n = LayerNorm(y) by linearity -- BasicTransformerBlock.ff.net.0 (reference unet1d/attention.py:178-203, GEGLU 206-301) of the blocks
 * whose hidden tensor does not fit the fused ns2vc_k_ffn.  128 tokens stay in registers, four workgroups per token block sweep a quarter of
 * the hidden units each; out_op [M][ldo] (>= 4 dim columns) operand-typed.  yn = the RAW operand copy of y [M][ldy]; ln_stats as in
 * ns2vc_gemm_args.ln_stats ([M][dim/64] (sum, sumsq)); wstream / consts from ns2vc_pack_geglu. */
typedef struct ns2vc_geglu_args {
  const void* yn; int32_t ldy;
  const float* ln_stats; float ln_eps;
  const void* wstream; const float* consts;
  void* out_op; int32_t ldo;
  int32_t M, dim;
  unsigned* ln_health;                      /* optional, as in ns2vc_gemm_args */
  /* Per-item frame counts (backward-compatible addition to ABI v7: the two fields are the LAST of the struct, a zero-filled tail = everything above
   * as it was).
   *   T    = frames per item, any value >= 1 with M % T == 0 (read only when `lens` is set);
   *   lens = DEVICE [B], B = M / T entries, one count per batch item.  Row m is frame t = m - b T of item b = m / T and takes part iff t < lens[b];
   *          a count is clamped to 0 .. T before it is used.
   * A row at or past its item's end: its `yn` and `ln_stats` rows are not read, it takes no part in ln_health, and its out_op row (the 4 dim
   * columns) is stored as exact zeros.  Rows at or past M stay unwritten.  A 128-row block without a valid row stores its zeros and returns: no
   * weight is streamed for it.
   * Statistics under `lens`: with ln_stats given they are used exactly as without lengths -- every valid row is bit-identical to the launch without
   * `lens` on its item alone at M = lens[b].  With ln_stats == NULL (allowed only together with `lens`) the kernel takes (sum, sum of squares) from
   * the token's ROUNDED operand row `yn`, which it holds in registers: no row-statistics producer is needed.  The two modes agree to about 0.1
   * operand ulp in relative L2 and are equally close to the exact LayerNorm of the unrounded row, but they are not bit-comparable with each other.
   * Served by the masked instantiations of the kernel (both operand types).  A call that sets `lens` with T < 1 or M % T != 0, or that leaves
   * ln_stats NULL without `lens`, is refused (hipErrorInvalidValue), never run unmasked.
   * The struct is 16 bytes longer than in earlier builds of ABI v7 and ns2vc_k_geglu reads all of it: a binding compiled against the earlier header
   * MUST be rebuilt; ns2vc_sizeof_geglu_args() is there to check. */
  int32_t T;
  const int32_t* lens;
} ns2vc_geglu_args;
/* w1_packed [8*dim][dim], bias1_packed [8*dim] (or NULL): LayerNorm-folded ff.net.0 rows / bias in the packed (32 value | 32 gate) order,
 * fp32 host.  Returns the device tile stream and the device constants ((rowsum of the rounded row, bias) per stream row). */
int ns2vc_pack_geglu(const float* w1_packed_host, const float* bias1_packed_host, int dim, int precision, void** out_stream_dev, float** out_consts_dev);
int ns2vc_k_geglu(const ns2vc_geglu_args* a, int precision, void* stream);
/* the same packing on the host only (no GPU needed; tests): stream_out [8*dim*dim] operand-typed bit patterns in consumption order
 * ([quarter][unit block][K tile][128 rows][64 k], rows of every 32-unit group permuted, 16-byte chunks XOR-swizzled), consts_out [8*dim][2] */
int ns2vc_pack_geglu_host(const float* w1_packed_host, const float* bias1_packed_host, int dim, int precision, uint16_t* stream_out, float* consts_out);

/* Two token-local GEMMs with a LayerNorm in between, in one launch (csrc/rowchain.hip; 16-bit precisions, dim 128 / 256):
 *   y = A W1^T + bias1 (+ res)  -> out1_f32 (optional);   z = LayerNorm(y) W2'^T + b2'  -> out2_op   (gamma/beta folded into W2' / b2')
 * Replaces Transformer2DModel.proj_in + BasicTransformerBlock.norm1 + attn1.to_q|to_k|to_v (transformer_1d.py:270-279,
 * attention.py:130-140; n2 = 3 dim) and attn1.to_out + residual + norm2 + attn2.to_q (attention_processor.py:1040-1050,
 * attention.py:141-160; n2 = dim).  a_op [M][lda] operand rows; wstream from ns2vc_pack_rowchain; consts2 [n2][2] =
 * (sum_k of the rounded W2' row, folded bias).  res may alias out1_f32 element for element. */
typedef struct ns2vc_rowchain_args {
  const void* a_op; int32_t lda;
  const void* wstream; const float* bias1; const float* consts2;
  const float* res; int32_t ldres;          /* optional fp32 residual added to y */
  float* out1_f32; int32_t ldo1;            /* fp32 y, or NULL */
  void* out2_op; int32_t ldo2;              /* operand-typed z [M][ldo2] */
  float ln_eps; int32_t M, dim, n2;
  unsigned* ln_health;                      /* optional, as in ns2vc_gemm_args */
  /* optional GroupNorm prologue: A = GroupNorm(gn_x) (affine, no activation) built inside the kernel; a_op is ignored.
   * gn_x fp32 [M][ldx]; gn_stats = the producer's per-(batch item, 16-channel block) int64 (sum, sumsq) as left by
   * ns2vc_gemm_args.stats; gn_gamma / gn_beta [dim]; T = rows per batch item (>= 64); G = groups (dim/G a multiple of 16) */
  const float* gn_x; int32_t ldx;
  const long long* gn_stats; const float* gn_gamma; const float* gn_beta;
  float gn_eps; int32_t T, G;
  /* r4: N-sliced stage 2 (dim 384): `slices` = 2 -> two workgroups per token block, each repeats stage 1 and computes one slice of the stage-2
   * rows (5 + 4 of the 9 row blocks of q|k|v, 2 + 1 of the 3 of to_q); wstream / consts2 from ns2vc_pack_rowchain_sliced.  0 / 1 = one workgroup. */
  int32_t slices;
  /* Per-item frame counts (backward-compatible addition to ABI v7: the LAST field of the struct, NULL = everything above as it was).
   *   lens = DEVICE [M / T], one count per batch item; `T` = rows per item is then required with or without the GroupNorm prologue (T >= 1 and
   *          M % T == 0; T >= 64 with the prologue, as before).  Row m is frame t = m - b T of item b = m / T and takes part iff t < lens[b]; a
   *          count is clamped to 0 .. T before it is used.
   * A row at or past its item's end: out1_f32 and out2_op are stored as exact zeros (no bias, no residual, no LayerNorm fix-up), whatever a_op / gn_x
   * hold there; its `res` row is not read; it takes no part in ln_health.  Every other row is bit-identical to the launch on its item alone at
   * M = lens[b]; with the GroupNorm prologue gn_stats hold the sums over the item's valid rows only (as ns2vc_gemm_args.lens leaves them) and the
   * divisor is lens[b] * dim / G.  Served by the masked instantiations of the kernel: both operand types, every dim and n2, 128-token blocks and
   * two slices included.  A call that sets `lens` with T < 1, M % T != 0 or a prologue at T < 64 is refused (hipErrorInvalidValue), never run unmasked.
   * The struct is 8 bytes longer than in earlier builds of ABI v7 and ns2vc_k_rowchain reads all of it: a binding compiled against the earlier
   * header MUST be rebuilt; ns2vc_sizeof_rowchain_args() is there to check. */
  const int32_t* lens;
} ns2vc_rowchain_args;
/* w1 [dim][dim], w2 [n2][dim]: fp32 host, row-major.  Returns the device tile stream the kernel consumes. */
int ns2vc_pack_rowchain(const float* w1_host, const float* w2_host, int dim, int n2, int precision, void** out_stream_dev);
int ns2vc_pack_rowchain_sliced(const float* w1_host, const float* w2_host, int dim, int n2, int slices, int precision, void** out_stream_dev);
int ns2vc_k_rowchain(const ns2vc_rowchain_args* a, int precision, void* stream);
int ns2vc_debug_set_geglu_min_rows(int rows); /* tests / tuning: row count from which the planner picks ns2vc_k_geglu over the GEMM (default 4608; < 0 restores it); takes effect at the next plan build */
int ns2vc_debug_set_attn_keys(int keys); /* tests / tuning: 128 selects the 128-key K/V tile kernels (16-bit precisions, hd 16 / 32); 0 or 64 = the default 64-key tiles */
int ns2vc_debug_set_attn_optimistic(int on); /* tests: 0 = every attention workgroup takes the exact (per-tile maximum) pass only; 1 = default */
int ns2vc_debug_set_attn_resident(int mode); /* tests / tuning: the K/V-resident attention kernel (dense fp16 / bf16, hd 16 / 32, <= 1024 / 640 keys): -1 = the rule (B * H >= the device's CUs; default), 0 = never, 1 = whenever the launch fits */
unsigned long long ns2vc_debug_attn_resident_launches(void); /* tests: attention launches issued (or captured into a graph) on the resident kernel so far in this process */
int ns2vc_debug_attnres_table(int* rows); /* rows of the resident attention kernel's table (not a family of ns2vc_debug_kernel_table); no HIP call */
int ns2vc_debug_set_attn_resident_lens(int mode); /* tests / tuning: the resident kernel's masked form for launches with q_lens / k_lens (fp16 / bf16, hd 16 / 32, padded Lk <= 1024 / 640): -1 = the rule (B * H >= the device's CUs; default), 0 = never, 1 = whenever the launch fits */
unsigned long long ns2vc_debug_attn_resident_lens_launches(void); /* tests: attention launches issued (or captured into a graph) on the resident kernel's masked form so far in this process */
int ns2vc_debug_attnres_lens_table(int* rows); /* rows of that form's table (not a family of ns2vc_debug_kernel_table); no HIP call */
int ns2vc_debug_set_rowchain_tokens(int nt); /* tests: force 64-token (1) / 128-token (2, dim 128 only) workgroups; 0 = heuristic */

/* operand-typed conversions for tests: fp32 host [n] -> device operand buffer and back */
int ns2vc_to_operand(const float* host, size_t n, int precision, void** out_dev);
int ns2vc_from_operand(const void* dev, size_t n, int precision, float* host);
/* the host-side rounding used for weight packing (round to nearest even; fp16 overflow -> inf): host in, host out, no GPU needed */
int ns2vc_round_to_operand(const float* host_in, size_t n, int precision, float* host_out);
int ns2vc_pack_weight(const float* rows_host, int N, int K, int precision, void** out_dev); /* [N][K] fp32 host -> device, engine dtype */
int ns2vc_k_gemm(const ns2vc_gemm_args* a, int precision, void* stream);
/* ABI v6: rows [N][3 * ctot + c2] fp32 host (k = tap * ctot + c, then the c2 columns of a fused 1x1 segment) -> device, engine dtype, N padded to 128,
 * tile-major: [N / 64][steps][64 rows][128 B] in the tap-sharing kernel's step order, pre-swizzled (csrc/convts.hip pack_conv3_tiled). */
int ns2vc_pack_conv3_tiled(const float* rows_host, int N, int ctot, int c2, int precision, void** out_dev);
int ns2vc_weight_rowsum(const float* rows_host, int N, int K, int precision, float** out_dev); /* [N] fp32: sum_k round_to_operand(rows[n][k]) */
int ns2vc_debug_set_gemm_trace(void* dev_u64_blocks_x8); /* tuning: per-workgroup s_memtime stamps of the next GEMM launches; NULL = off */
int ns2vc_debug_poison(unsigned pattern, int lds_bytes, void* stream); /* test tool: leave `pattern` in every CU's LDS (first lds_bytes) and in vector registers, as a foreign kernel would */
/* ABI v6 (diagnostic): where the 256-thread blocks of an n_blocks launch on `stream` ran: out_host[2 i] = XCC id (HW_REG_XCC_ID),
 * out_host[2 i + 1] = HW_REG_HW_ID of block i; `spin` > 0 keeps blocks resident for a while so the grid spreads over the CUs the stream may use. */
int ns2vc_debug_placement(void* stream, int n_blocks, int spin, uint32_t* out_host);
int ns2vc_debug_kernel_table(int family, int* rows, int* unready); /* tests: the instantiation table of one kernel template (0 gemm2, 1 gemm4, 2 conv3ts, 3 attn, 4 ffn, 5 geglu, 6 rowchain). *rows = its row count (no device needed).  With unready != NULL the family's attribute setup runs, and *unready = the rows whose function reports less dynamic LDS than the row needs, or that need more than 160 KB */
int ns2vc_debug_set_gemm_tile(int bm, int bn, int stages); /* force the GEMM tile: stages 2..4 = 4-wave kernel ring depth, 12|13 = 8-wave K-split kernel ring 2|3; 0,0,0 = heuristic; (-1,0,0) = heuristic without the loader/consumer tiles, (-2,0,0) = with them again; ABI v6: (128, 64|128, 54|58) = the tap-sharing conv kernel with 4|8 loader waves (k = 3 launches only), (-3,0,0) = never that kernel, (-4,0,nl) = heuristic with it again, nl loader waves (0 = default) */
int ns2vc_k_attention(const ns2vc_attn_args* a, int head_dim, int precision, void* stream);
/* GroupNorm (+ optional resnet time scale/shift, + optional SiLU) of a (possibly concatenated) fp32 tensor,
 * written as an operand tensor [B*T][c0+c1]; raw_op (optional) receives the un-normalised concat. Synchronous. */
int ns2vc_k_groupnorm(const float* a0, int lda0, int c0, const float* a1, int lda1, int c1, int B, int T, int G, float eps,
                      const float* gamma, const float* beta, const float* temb, int ldtemb, int temb_off, int silu,
                      void* out_op, void* raw_op, int precision, void* stream);
/* the engine's form of the same launch: statistics = the int64 fixed-point sums a producer GEMM's epilogue left
 * (ns2vc_gemm_args.stats, [B][c0/16][2]); one source, asynchronous on `stream`.  What ns2vc_gemm_args.gnp_* reproduces bit for bit. */
int ns2vc_k_groupnorm_stats(const float* a0, int lda0, int c0, const long long* stats0, int B, int T, int G, float eps, const float* gamma,
                            const float* beta, const float* temb, int ldtemb, int temb_off, int silu, void* out_op, int precision, void* stream);
/* ABI v5: the same for the channel concat of two tensors (the up blocks' torch.cat([h, skip])), each with its own statistics, plus the
 * optional un-normalised operand copy.  What ns2vc_gemm_args.gnp_x1 / gnp_raw reproduce bit for bit. */
int ns2vc_k_groupnorm_stats2(const float* a0, int lda0, int c0, const long long* stats0, const float* a1, int lda1, int c1, const long long* stats1,
                             int B, int T, int G, float eps, const float* gamma, const float* beta, const float* temb, int ldtemb, int temb_off,
                             int silu, void* out_op, void* raw_op, int precision, void* stream);
/* LayerNorm without affine (gamma/beta are folded into the consumer's weights): fp32 rows -> operand rows */
int ns2vc_k_layernorm_apply(const float* x, int ldx, int M, int C, float eps, void* out_op, int precision, void* stream);
int ns2vc_k_nct_to_btc(const float* src, int C, int T, int B, float* dst, int ldd, int cpad, void* stream);
int ns2vc_k_btc_to_nct(const float* src, int lds, int C, int T, int B, float* dst, void* stream);
/* the normals a stochastic update adds at table row `step`: out = fp32 rows [B*T][ld] (ld % 4 == 0) channels-last, out[(b*T + t)*ld + c] = z for
 * c < C and t < lens_dev[b] (lens_dev = DEVICE [B] or NULL = all T), 0 elsewhere; seeds_dev = DEVICE [B] */
int ns2vc_k_noise(const uint64_t* seeds_dev, int B, int C, int T, int ld, int step, const int32_t* lens_dev, float* out, void* stream);
/* One solver update of the sampling loop (backward-compatible addition to ABI v7), the launch ns2vc_sampler_steps makes after every
 * evaluation: row *step_dev of coef_dev (DEVICE [steps][NS2VC_NCOEF], ns2vc_amd.schedule.build_table) applied to x0 and the fp32 state
 * xe, xbar, d1, mprev (rows [n / ld][ld], updated in place; ns2vc_amd/schedule.py states the recurrence).  xe_op receives the new xe in the
 * operand type: fp32 rows [n / ld][ld], or for 16-bit precisions the hi + lo pair [hi(ld) | lo(ld)], row stride 2 * ld.
 * mprev2 = NULL: the order <= 2 update (columns 10-11 ignored).  Non-NULL: the history-2 update of order-3 tables, which reads m_{i-2}
 * there and leaves m_{i-1}.  No noise term (stochastic tables run only inside the loop). */
int ns2vc_k_solver_update(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                          float* d1, float* mprev, float* mprev2, size_t n, int ld, void* stream);
/* The guided form of that launch (backward-compatible addition to ABI v7; the combination of sampler/uni_pc.py:225-229 and
 * sampler/dpm_solver.py:327-331 in x0 space, see ns2vc_sampler_set_guidance): a batch of 2n items of T rows of ld columns, rows [0, n*T)
 * unconditional and [n*T, 2n*T) conditional.  n_half = n * T * ld, the elements of ONE half; x0, xe and xe_op cover both halves, xbar, d1,
 * mprev and mprev2 the first only.  Element e of the first half: x0_g = scale_dev[b] == 1 ? x0[e + n_half] : x0[e] + scale_dev[b] * (x0[e + n_half] - x0[e])
 * with b = (e / ld) / T, then the update of ns2vc_k_solver_update; the new xe and its operand copy go to both halves (pair row r + n*T).
 * seeds_dev (DEVICE [n], optional): the noise term of stochastic rows as the loop adds it, on channels c < nc and frames t < lens_dev[b]
 * (DEVICE [n] or NULL = all T); not with mprev2.  Refused, never run unguided: T <= 0, n_half not a multiple of T * ld, ld not a multiple of 4. */
int ns2vc_k_solver_update_guided(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                                 float* d1, float* mprev, float* mprev2, size_t n_half, int ld, const float* scale_dev, int T, const uint64_t* seeds_dev,
                                 const int32_t* lens_dev, int nc, void* stream);
/* The quantile launch of the dynamic thresholding (backward-compatible addition to ABI v7) on ready values: thr[b] = torch.quantile(|v_b|, p) in
 * its float32 rule (ns2vc_amd.schedule.abs_quantile), v_b = rows t < lens_dev[b] (DEVICE [n_items] or NULL = all T; clamped to [0, T]) and
 * columns c < nc of item b's T rows of ld columns of `values` (fp32, 16-byte aligned, ld % 4 == 0).  Exact: a radix select over the bit patterns,
 * integer counts only.  thr = DEVICE [n_items]; an item without elements gives 0.  NaN / Inf among the values: unspecified result, nothing else. */
int ns2vc_k_abs_quantile(const float* values, int n_items, int T, int ld, int nc, const int32_t* lens_dev, float p, float* thr, void* stream);
/* One corrected solver update as the loop makes it (backward-compatible addition to ABI v7; see ns2vc_sampler_set_x0_correction): mode 1 = the
 * quantile launch on m formed from x0, xe and row *step_dev (guided_x0 of the halves first when scale_dev is set), thr_dev[b] = that quantile
 * (DEVICE [n_items], n_items = n / (T * ld)), then the update with m = clamp(m, -s_b, s_b) / s_b, s_b = max(thr_dev[b], max_val); mode 2 = the
 * update with m = clamp(m, -max_val, max_val), thr_dev unused.  scale_dev = NULL: the arguments of ns2vc_k_solver_update, n = all elements;
 * non-NULL: those of ns2vc_k_solver_update_guided, n = the elements of ONE half.  lens_dev / nc: the elements the quantile runs over.  No noise. */
int ns2vc_k_solver_update_corrected(const float* coef_dev, const int32_t* step_dev, const float* x0, float* xe, void* xe_op, int precision, float* xbar,
                                    float* d1, float* mprev, float* mprev2, size_t n, int ld, int T, const float* scale_dev, const int32_t* lens_dev,
                                    int nc, int mode, float ratio, float max_val, float* thr_dev, void* stream);
/* One solver update under per-item schedules as the loop makes it (backward-compatible addition to ABI v7; see ns2vc_sampler_load_items):
 * items_host = HOST [n_items][4] int32 records (row0, steps, start, flags: 1 = history 2, 2 = noise) into coef_dev of n_rows rows, checked
 * here and copied to the device by the call, which also waits for `stream` (a test hook).  At loop step r = *step_dev item b is active when
 * 0 <= r - start < steps and gets the update of ns2vc_k_solver_update (flags 1: its history-2 form; 2: with the noise term, Philox row word
 * r - start) / _guided (scale_dev set: n = the elements of ONE half) / _corrected (mode 1 | 2) on row row0 + r - start; every other item keeps
 * every bit of xe, xe_op, xbar, d1, mprev, mprev2 and thr_dev[b].  n = n_items * T * ld. */
int ns2vc_k_solver_update_items(const float* coef_dev, int n_rows, const int32_t* step_dev, const int32_t* items_host, int n_items, const float* x0, float* xe,
                                void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, size_t n, int ld, int T,
                                const float* scale_dev, const uint64_t* seeds_dev, const int32_t* lens_dev, int nc, int mode, float ratio, float max_val,
                                float* thr_dev, void* stream);
/* The same step under a per-item x0 correction (backward-compatible addition to ABI v7; see ns2vc_sampler_set_x0_correction_items): the arguments of
 * ns2vc_k_solver_update_items with mode, ratio, max_val replaced by HOST arrays [n_items] of each, validated as that call validates them (a
 * stochastic item takes mode 0 only).  The two launches the loop makes: the per-item quantile when a record has mode 1 (thr_dev[b] is written for
 * the active items in mode 1 and for no other), then the update, every active item by its own record.  thr_dev is always needed. */
int ns2vc_k_solver_update_items_corrected(const float* coef_dev, int n_rows, const int32_t* step_dev, const int32_t* items_host, int n_items, const float* x0,
                                          float* xe, void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, size_t n, int ld, int T,
                                          const float* scale_dev, const uint64_t* seeds_dev, const int32_t* lens_dev, int nc, const int32_t* mode_host,
                                          const float* ratio_host, const float* max_val_host, float* thr_dev, void* stream);

/* ---- Slot loop: continuous batching (backward-compatible additions to ABI v7) --------------------------------------------------
 * A loop over a prepared (B, T, Lp) engine whose loop items (B; n under guidance) are SLOTS that are filled, run and emptied independently while
 * the captured step graph keeps replaying.  A request admitted into slot b with start = r runs rows 0 .. steps-1 of its own table at loop steps
 * r .. r+steps-1 and ends on the bits it gets when the same engine shape runs it in the same slot from loop step 0 with the other slots idle;
 * the other slots keep the bits they would have had without the admission.  Every call below is asynchronous on `stream` (host data travels
 * through pinned staging; use ONE stream for a loop) and none ends the loop.  ns2vc_sampler_open is where buffers are allocated (records,
 * slot lists for all B items, m_prev2, seeds, thresholds): it may wait for the device when one has to grow.  The calls of a running loop
 * (_write_rows, _admit, _take, _rebase, ns2vc_unet_set_condition_items in slot mode) allocate nothing and never wait for the device; the
 * host blocks only when it is eight calls ahead of the copies out of its staging ring.  Outside slot mode
 * ns2vc_unet_set_condition_items allocates its slot list on first use and waits for `stream` when the list has to grow.
 *
 * ns2vc_sampler_open: puts the prepared engine into slot mode.  Every slot starts IDLE: record {row0 0, steps 1, start INT32_MAX, flags 0} --
 * never active, evaluated at row 0 --, state (xe, its operand copy, xbar, d1, mprev, mprev2) zero, content and prompt rows zero with the
 * hoisted tensors rebuilt from them, the 1024-row coefficient table zero (model time 0), its timestep-embedding table rebuilt: all finite.
 * The step counter runs from 0.  What the captured step graph bakes in is fixed here: history2 != 0 = items with order-3 tables may come
 * (m_prev2 is allocated), noise != 0 = stochastic items may come (the seeds buffer is allocated; not with the x0 correction); guidance and the
 * x0 correction are the engine's settings at this moment.  Admissions within these forms never recapture (ns2vc_unet_graph_captures stays).
 * Step counter rule: loop steps are 32-bit; a call that would pass 2^31 - 2 is refused.  ns2vc_sampler_rebase on a loop whose slots are all
 * idle sets the counter back to 0 and does nothing else -- no recapture; table, condition and state stay (an idle record is active at no step).
 * Opening again starts afresh (refused while slots are busy).  Refused with option fuse_solver.  ns2vc_sampler_handoff refuses a slot loop; ns2vc_sampler_load / _load_items refuse while slots are busy
 * and otherwise leave slot mode; ns2vc_sampler_begin leaves it (and fails: a table must be loaded first); ns2vc_sampler_end ends it.
 * In slot mode ns2vc_sampler_steps is not bounded by a table length (idle steps are legal) and ns2vc_sampler_peek gives all loop items.
 * Legal in mid-loop, each a stream-ordered copy that replays the captured graph: ns2vc_unet_set_lengths and ns2vc_unet_set_prompt_lengths
 * (while they stay ON: switching either on or off rebuilds the plan and recaptures), ns2vc_sampler_set_seeds, ns2vc_sampler_set_guidance
 * (new scales; on / off ends the loop), ns2vc_sampler_set_x0_correction_items (new records while the table is on: a loop opened with the table
 * takes corrected and stochastic items side by side).  They take whole vectors: change the entries of idle slots only, or a running item changes course. */
int ns2vc_sampler_open(ns2vc_unet* h, int history2, int noise, void* stream);
int ns2vc_sampler_rebase(ns2vc_unet* h, void* stream);
/* rows [row0, row0 + nrows) of the 1024-row coefficient table <- coef_host [nrows][NS2VC_NCOEF] (finite), and the same rows of the
 * timestep-embedding table (a row's embedding depends on that row alone: every other row keeps its bits).  Refused while a busy slot that has
 * not finished walks any of the rows.  Which tables live where is the caller's business (ns2vc_amd.schedule.TablePool). */
int ns2vc_sampler_write_rows(ns2vc_unet* h, int row0, int nrows, const float* coef_host, void* stream);
/* n idle slots (HOST list, no repeats) take x_T_nct = DEVICE [n][C][T] and records = HOST [n][4] int32 {row0, steps, start, flags (1 = history 2,
 * 2 = noise: must equal the form of the rows)} with start >= the current loop step.  ONE launch writes, for the listed slots only, exactly
 * what ns2vc_sampler_begin leaves for those items (xe fp32 with pad channels and rows past lengths[slot] zero, the operand copy incl. the
 * [hi | lo] pair of 16-bit engines, xbar = xe, d1 = mprev = mprev2 = 0; guided: xe and the operand copy also in slot + n, whose xbar rows are
 * zero) and the slots' records; the slot list is read from device memory.  Set the slot's lengths, condition, seed and scale BEFORE it. */
int ns2vc_sampler_admit(ns2vc_unet* h, int n, const int32_t* slots, const float* x_T_nct, const int32_t* records, void* stream);
/* the slot-list form of ns2vc_sampler_peek: xe of n finished busy slots -> x_out_nct = DEVICE [n][C][T], one launch, which also makes the
 * slots idle (their records; the state stays as it is, finite). */
int ns2vc_sampler_take(ns2vc_unet* h, int n, const int32_t* slots, float* x_out_nct, void* stream);
int ns2vc_sampler_slot_step(ns2vc_unet* h, int* loop_step); /* the loop step the next ns2vc_sampler_steps starts at; -1 = no slot loop */
/* content_nct = DEVICE [n][content][T], prompt_nlc = DEVICE [n][Lp][cross], mask_nl = DEVICE [n][Lp] or NULL -> items slots[k] of the prepared
 * B (a guided engine: both halves are the caller's business), as ns2vc_unet_set_content / _set_prompt write them for the whole batch (NCT ->
 * channels-last, operand or hi + lo copy, rows past lengths[slot] zero), by ONE scatter launch; then the whole condition plan runs again: the
 * other items' hoisted tensors keep their bits.  A mask needs a plan built with one (NULL then keeps every key).  Works in and out of slot mode. */
int ns2vc_unet_set_condition_items(ns2vc_unet* h, int n, const int32_t* slots, const float* content_nct, const float* prompt_nlc, const uint8_t* mask_nl,
                                   void* stream);
/* test hooks of the two state kernels: slots_host = HOST [n] in [0, n_items); buffers as ns2vc_k_solver_update_items takes them (n_items items of
 * T rows of ld columns; guided != 0: 2 * n_items items in xe / xe_op / xbar / d1 / mprev / mprev2); lens_dev = DEVICE [n_items] or NULL.  Both wait
 * for `stream`.  No records are written. */
int ns2vc_k_sampler_admit(const float* x_T, int C, int T, int n, const int32_t* slots_host, int n_items, float* xe, void* xe_op, int precision, float* xbar,
                          float* d1, float* mprev, float* mprev2, int ld, const int32_t* lens_dev, int guided, void* stream);
int ns2vc_k_sampler_take(const float* xe, int ld, int C, int T, int n, const int32_t* slots_host, int n_items, float* out, void* stream);
/* The hold launch of ns2vc_sampler_set_known on its own (backward-compatible addition to ABI v7; a test hook, waits for `stream`).  x0 = DEVICE
 * fp32 rows [halves * n * T][ld], known_rows = DEVICE fp32 rows [n * T][ld] channels-last (ld % 4 == 0, both 16-byte aligned), mask_host = HOST
 * [n][T] uint8.  Rows: row r = b * T + t with mask_host[b][t] != 0 is held, no other row is touched.  Columns: x0[r][c] = known_rows[r][c] bit for
 * bit for c < nc; the pad columns nc <= c < ld of a held row are written as zero whatever known_rows holds there.  Halves: halves = 2 (a guided
 * engine: n * T unconditional rows, then n * T conditional rows) writes the same values to rows r and r + n * T; halves = 1 to row r alone. */
int ns2vc_k_hold_x0(float* x0, const float* known_rows, const uint8_t* mask_host, int n, int T, int ld, int nc, int halves, void* stream);

/* ---- Known frames in a slot loop (backward-compatible additions to ABI v7) -----------------------------------------------------
 * ns2vc_sampler_open_known: ns2vc_sampler_open, and in addition every SLOT gets known-frame state for the whole prepared shape, outside the plan
 * arena: known rows [loop items * T][padded channels] fp32, channels-last like x0, and one mask byte per frame, all clear.  The captured step
 * then has one more launch between the plan's last launch and the solver update: one wave per 64 consecutive rows b * T + t reads 64 mask bytes,
 * returns when none is set, and otherwise copies the held rows from the known rows into x0 (pad columns zero, both halves of a guided engine) --
 * ns2vc_sampler_set_known's rule, with the rows given by the mask instead of a list, so an admission changes its own slot's bytes only and never
 * recaptures.  The form is part of the step graph: opening with it after a loop without it (or the other way round, by a later plain
 * ns2vc_sampler_open) captures again.  Refused: a loop-wide x0 correction or the per-item correction table being on (a correction would rescale
 * held frames; the two setters refuse while such a loop is open), and a closed-loop hold that is on (ns2vc_sampler_set_known), as
 * ns2vc_sampler_open refuses it.  ns2vc_sampler_end ends the slots' known frames with the loop (the host mirror goes, the next open clears every
 * mask) but leaves the form baked, so that the next ns2vc_sampler_open_known replays the step graph; a step run in between is refused.
 * ns2vc_unet_prepare, ns2vc_sampler_load / _load_items / _begin (which leave slot mode) and a change of guidance on / off drop the form too,
 * and with it the step graph.  ns2vc_sampler_handoff and option fuse_solver refuse slot loops as before.
 *
 * ns2vc_sampler_set_known_items: the known frames of n listed IDLE slots (HOST list, no repeats; n counts loop items under guidance).  known_nct =
 * DEVICE fp32 [n][latent][T], mask_nt = HOST [n][T] bytes (nonzero = held).  The mask travels through the slot loop's pinned staging ring and ONE
 * launch, which reads the slot list from device memory, transposes the latent into the slots' known rows and writes their mask bytes: the call
 * never waits for the device and never allocates.  Both NULL clears the listed slots' masks.  Set the slots' lengths first.  Refused: no slot loop,
 * or one opened without the form; a busy slot; a slot outside the range; a held frame at or past the slot's applied length (ns2vc_sampler_admit
 * checks again, against a host mirror of each slot's last held frame, so lengths set afterwards are caught).  A slot's known frames last for
 * exactly ONE request: in a loop of this form ns2vc_sampler_take clears the masks of the slots it takes, by a second launch in the same call. */
int ns2vc_sampler_open_known(ns2vc_unet* h, int history2, int noise, void* stream);
int ns2vc_sampler_set_known_items(ns2vc_unet* h, int n, const int32_t* slots, const float* known_nct, const uint8_t* mask_nt, void* stream);
/* test hooks of the two kernels; both wait for `stream`.
 * ns2vc_k_hold_slots: the step's launch alone.  x0 = DEVICE fp32 rows [halves * n * T][ld], known_rows = DEVICE fp32 rows [n * T][ld] (ld % 4 == 0,
 * both 16-byte aligned), mask_host = HOST [n][T] bytes, copied to the device for the call.  Row r = b * T + t with a nonzero byte: x0[r][c] =
 * known_rows[r][c] for c < nc, zero for nc <= c < ld, also in row r + n * T where halves = 2; every other byte of x0 is left alone.
 * ns2vc_k_known_items: known_nct = DEVICE fp32 [n][C][T] and mask_host = HOST [n][T] bytes -> rows [slot * T, + T) of known_rows = DEVICE fp32
 * [nslots * T][ld] (columns C .. ld zero) and of mask_dev = DEVICE [nslots * T] bytes (0 | 1) for slot = slots_host[k]; an entry outside
 * [0, nslots) is skipped; known_nct = mask_host = NULL: the listed slots' bytes of mask_dev become zero and known_rows is not touched. */
int ns2vc_k_hold_slots(float* x0, const float* known_rows, const uint8_t* mask_host, int n, int T, int ld, int nc, int halves, void* stream);
int ns2vc_k_known_items(const float* known_nct, const uint8_t* mask_host, int C, int T, int n, const int32_t* slots_host, int nslots, float* known_rows,
                        uint8_t* mask_dev, int ld, void* stream);

/* ---- Suspend and resume of a slot's request (backward-compatible additions to ABI v7) -------------------------------------------
 * A busy slot's request is its SOLVER STATE -- the engine's fp32 rows xe, xbar, d1, mprev and, in a loop opened with history2, mprev2: P = 4 or 5
 * planes of T channels-last rows of ld = padded channels columns each (under guidance the first half's rows; xe of the second half is the same
 * point) -- and its POSITION done = loop step - start = the rows of its table already run.  Condition, lengths, seed, scale, correction record and
 * known frames are not state: the caller holds them and sets them again before a resume, exactly as before an admission.
 * ns2vc_sampler_state_shape: P, T and ld of the open slot loop; a state buffer is DEVICE fp32 [n][P][T][ld], 16-byte aligned.
 * ns2vc_sampler_suspend: the planes of n busy slots (HOST list, no repeats) -> state_out_dev bit for bit (pad columns and rows past the length
 * included), done_out_host[k] = the slot's position, and the slots become idle (records; in a loop with known frames their masks are cleared, as
 * ns2vc_sampler_take clears them).  Only a slot with 0 <= done < steps: an idle slot, one that has not started and one that has finished (take it)
 * are refused.
 * ns2vc_sampler_resume: state_in_dev -> n IDLE slots of this or another engine of the same T, ld and loop form, records = HOST [n][4] int32 {row0,
 * steps, done, flags}, 0 <= done < steps.  ONE launch writes the planes back, rebuilds the operand copy of xe as the solver update stores it ([hi |
 * lo] pair of 16-bit engines included), writes xe and its operand copy into slot + n of a guided engine and zeroes that item's xbar and history
 * rows as ns2vc_sampler_admit does, and installs the record {row0, steps, start = loop step - done, flags}: the slot's next step runs row row0 +
 * done, and a stochastic item continues its own noise stream (the Philox row word is the local row).  start lies in the past and may be negative
 * after ns2vc_sampler_rebase.  The rows may sit at another row0 than before.  Refusals are those of ns2vc_sampler_admit (rows never written, flags
 * that differ from the rows' form, a history-2 or stochastic record in a loop opened without it, guided halves of different lengths, a known frame
 * at or past the length, a busy slot) plus done outside [0, steps).
 * A request suspended at any done and resumed into the same slot index ends on the bits of the uninterrupted run, whatever the slot did in
 * between; the other slots keep theirs.  Neither call recaptures the step graph, allocates, or waits for the device. */
int ns2vc_sampler_state_shape(ns2vc_unet* h, int* planes, int* T, int* ld);
int ns2vc_sampler_suspend(ns2vc_unet* h, int n, const int32_t* slots, float* state_out_dev, int32_t* done_out_host, void* stream);
int ns2vc_sampler_resume(ns2vc_unet* h, int n, const int32_t* slots, const float* state_in_dev, const int32_t* records, void* stream);
/* test hooks of the two kernels; both wait for `stream`.  Buffers as ns2vc_k_sampler_admit takes them (n_items items of T rows of ld fp32 columns,
 * ld % 4 == 0, 16-byte aligned; guided != 0: 2 * n_items items); mprev2 = NULL: 4 planes, else 5.  slots_host = HOST [n], sent as given: an entry
 * outside [0, n_items) is skipped.  rec_dev = DEVICE [n_items][4] int32 or NULL: suspend writes the idle record {0, 1, INT32_MAX, 0} of every listed
 * slot there, resume the slot's row of records_host = HOST [n][4] {row0, steps, start, flags} (given together with rec_dev). */
int ns2vc_k_sampler_suspend(const float* xe, const float* xbar, const float* d1, const float* mprev, const float* mprev2, int T, int ld, int n,
                            const int32_t* slots_host, int n_items, float* state_out, int32_t* rec_dev, void* stream);
int ns2vc_k_sampler_resume(const float* state_in, int T, int ld, int n, const int32_t* slots_host, int n_items, const int32_t* records_host, int32_t* rec_dev,
                           float* xe, void* xe_op, int precision, float* xbar, float* d1, float* mprev, float* mprev2, int guided, void* stream);

/* ---- The flat solver step (backward-compatible addition to ABI v7) -------------------------------------------------------------
 * One row of a solver table on a state that has no layout: n >= 1 fp32 elements in each of the planes xe, xbar, d1, mprev and (history 2) mprev2,
 * updated in place by the recurrence of ns2vc_amd/schedule.py.  This is the update the top-level `sampler` package (the reference's DPM_Solver /
 * UniPC classes) launches after every call of a model it cannot hand to the captured loop: ONE launch, enqueued on `stream`, no host wait.
 * coef_dev = DEVICE [n_rows][NS2VC_NCOEF] (schedule.build_table); the CALLER states n_rows, and row must lie in [0, n_rows) -- the library keeps no
 * record of a table it did not load.  model_out = what the model returned at xe, `kind` says what it is:
 *   0 x_start: m = the float32 round trip eps = (xe - alpha x0) / sigma, m = (xe - sigma eps) / alpha -- every plane then has the bits
 *     ns2vc_k_solver_update leaves in fp32;  1 noise: m = (xe - sigma eps) / alpha;  2 v: eps = alpha v + sigma xe;  3 score: eps = -sigma score;
 *   4 data: m = model_out as given (an x0 that was corrected on the way).
 * mprev2 = NULL: the order <= 2 update; non-NULL: the history-2 update of order-3 tables.  m_out non-NULL = FORM: m is written there and no
 * state plane is written (FORM, a correction of m by the caller, then kind 4 on it is the corrected step; without a correction the three give
 * the planes of the plain step bit for bit).  Pointers need 4-byte alignment only, each plane on a phase of its own: the kernel runs float4
 * where all planes share a 16-byte phase (scalar head and tail around it) and scalar otherwise, and an element's bits do not depend on which.
 * The grid has at most NS2VC_FLAT_MAX_BLOCKS blocks of 256 threads, so one trip covers NS2VC_FLAT_MAX_BLOCKS * 1024 elements.
 * Refused: a null state pointer, coef_dev or model_out, n == 0, an unknown kind, a row outside the table, a pointer off 4-byte alignment. */
#define NS2VC_FLAT_MAX_BLOCKS 1024
int ns2vc_k_solver_step_flat(const float* coef_dev, int n_rows, int row, int kind, const float* model_out, float* xe, float* xbar, float* d1,
                             float* mprev, float* mprev2 /* NULL: history 1 */, float* m_out /* non-NULL: FORM */, size_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NS2VC_HIP_H */
