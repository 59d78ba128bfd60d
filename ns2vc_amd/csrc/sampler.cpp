// The sampling loop: the solver table, the per-item noise seeds, one evaluation + solver update per step -- captured once as a hipGraph and
// replayed -- and the hand-off of the solver state between two engines.
#include "engine_internal.h"

#include <cmath>
#include <cstring>

using namespace ns2vc;

// Does a step fold its solver update into conv_out?  r6: when conv_out is the plan's last launch and runs on the tap-sharing kernel, the update happens in its epilogue
// (same arithmetic, element for element: common.h solver_upd) -- x0 is never written, the state tensors are read and written once instead of twice
bool ns2vc::solver_in_conv_out(ns2vc_unet* h, GemmArgs& g) {
  if (h->guide.on) return false;                       // (the epilogue has no guided form: fuse_solver is ignored under guidance)
  if (h->x0c.mode || h->x0c.items.on) return false;   // (nor a corrected one: the threshold needs the whole x0 first)
  if (!h->fuse_solver || h->debug || h->conv_out_idx < 0 || h->conv_out_idx != (int)h->fwd_ops.size() - 1) return false;
  // (masked plan: the update must see x0 with its padded rows zeroed -- conv_out's epilogue has not zeroed them -- so it stays a launch of its own)
  if (h->lens.masked) return false;
  if (h->conv_out_prec != h->prec) return false;      // (exact_io: conv_out runs in fp32 there, the operand copy of the state is 16-bit)
  if (h->stochastic) return false;                     // (the epilogue has no noise term: a stochastic table runs the stand-alone update)
  if (h->hist2.on) return false;                       // (nor an m_{i-2}: history-2 tables too)
  if (h->items.on) return false;                       // (nor per-item rows: per-item schedules too)
  if (h->hold.on) return false;                        // (known frames overwrite x0, which the fold never writes)
  g = h->conv_out_g;
  g.out_f32 = nullptr;
  g.sol_coef = h->coef_dev; g.sol_step = h->step_dev; g.sol_ncoef = NS2VC_NCOEF;
  g.sol_xe = h->xe; g.sol_xe_op = h->xe_op; g.sol_xbar = h->xbar; g.sol_d1 = h->d1; g.sol_mprev = h->mprev; g.sol_ld = h->CP; g.sol_op_pair = h->prec != PREC_F32;
  return gemm_uses_convts(g, h->conv_out_prec);
}

// Per-item x0 correction against per-item records, per item: a corrected record on a stochastic one is refused, the two may share a loop.
// rec = the n records about to hold, of a table of n_rows rows (the correction table off: nothing to check).
static int item_corrections_fit(ns2vc_unet* h, const SolverItem* rec, int n, int n_rows) {
  const auto& ic = h->x0c.items;
  if (!ic.on || !rec) return 0;
  if (ic.n != n) return fail("the per-item x0 correction holds %d records, the loop takes %d items: set it again (ns2vc_sampler_set_x0_correction_items)", ic.n, n);
  return solver_items_fit("item", rec, nullptr, n, n_rows, nullptr, nullptr, nullptr, 0, ic.host.data());
}

extern "C" {

int ns2vc_sampler_load(ns2vc_unet* h, int steps, const float* coef_host) {
  const int kMaxSteps = 1024;   // fixed capacity: the table pointer is baked into the captured graph
  if (!h || !coef_host || steps <= 0) return fail("bad sampler table");
  if (steps > kMaxSteps) return fail("at most %d solver steps are supported", kMaxSteps);
  if (h->in_slot_loop() && h->slots.any_busy())
    return fail("a slot loop with busy slots is running (ns2vc_sampler_open): a shared table would end their items; take them first (ns2vc_sampler_take)");
  h->slots.on = false;      // (a shared table leaves slot mode)
  h->shold.drop(h);
  if (!h->coef_dev) HIPCHK(hipMalloc((void**)&h->coef_dev, (size_t)kMaxSteps * NS2VC_NCOEF * sizeof(float)));
  HIPCHK(hipDeviceSynchronize());   // a previous loop may still be reading the table
  HIPCHK(hipMemcpy(h->coef_dev, coef_host, (size_t)steps * NS2VC_NCOEF * sizeof(float), hipMemcpyHostToDevice));
  {
    unsigned long long hsh = 1469598103934665603ull;
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(coef_host);
    for (size_t i = 0; i < (size_t)steps * NS2VC_NCOEF * sizeof(float); ++i) { hsh ^= pb[i]; hsh *= 1099511628211ull; }
    h->coef_hash = hsh;
  }
  h->steps = steps;
  h->temb_table_valid = false;
  h->next_step = -1;
  const int form = solver_table_form(coef_host, steps);
  const bool stochastic = (form & SOLVER_ITEM_NOISE) != 0, hist2 = (form & SOLVER_ITEM_HIST2) != 0;
  if (form == SOLVER_ITEM_BOTH) { h->steps = 0; return fail("a solver table with both a noise column and history 2 (columns 10-11) is not supported"); }
  // (the update's noise arguments and its history-2 form are baked into the captured step graph)
  if (stochastic != h->stochastic || hist2 != h->hist2.on || h->items.on) drop_step_graph(h);      // (... and so is the per-item form, which a shared table switches off)
  h->stochastic = stochastic;
  h->hist2.on = hist2;
  h->items.on = false;
  return 0;
}

// Per-item schedules: the distinct tables' rows back to back in the coefficient table, one record per loop item.  The table pointer and the
// records' pointer are baked into the captured step graph, their contents are not: new schedules of the same form replay it.
int ns2vc_sampler_load_items(ns2vc_unet* h, int n_tables, const int32_t* table_rows, const float* coef_host, int n_items, const int32_t* item_table,
                             const int32_t* item_start, void* stream) {
  const int kMaxRows = 1024;    // fixed capacity of the coefficient table and of the timestep-embedding table (ns2vc_sampler_load's)
  if (check_ready(h, true)) return 1;
  if (!table_rows || !coef_host || !item_table || !item_start || n_tables <= 0 || n_items <= 0) return fail("bad per-item sampler tables");
  if (n_items != h->loop_items())
    return fail("per-item schedules for %d items, the loop takes %d (the prepared batch; n under guidance: set the guidance first)", n_items, h->loop_items());
  if (h->in_slot_loop() && h->slots.any_busy())
    return fail("a slot loop with busy slots is running (ns2vc_sampler_open): new schedules would end their items; take them first (ns2vc_sampler_take)");
  h->slots.on = false;      // (closed per-item schedules leave slot mode)
  h->shold.drop(h);
  std::vector<int> row0(n_tables), flags(n_tables, 0);
  long rows = 0;
  for (int k = 0; k < n_tables; ++k) {
    if (table_rows[k] <= 0) return fail("table %d has %d rows", k, (int)table_rows[k]);
    row0[k] = (int)rows;
    rows += table_rows[k];
    if (rows > kMaxRows) return fail("the distinct solver tables of the batch hold more than %d rows together (the table's fixed capacity)", kMaxRows);
    flags[k] = solver_table_form(coef_host + (size_t)row0[k] * NS2VC_NCOEF, table_rows[k]);
    if (flags[k] == SOLVER_ITEM_BOTH)
      return fail("table %d has both a noise column and history 2 (columns 10-11): not supported", k);
  }
  std::vector<SolverItem> rec(n_items);
  int S = 0;
  bool any_noise = false, any_h2 = false;
  for (int b = 0; b < n_items; ++b) {
    const int k = item_table[b];
    if (k < 0 || k >= n_tables) return fail("item %d names table %d of %d", b, k, n_tables);
    if (item_start[b] < 0 || item_start[b] > kMaxRows) return fail("item %d starts at loop step %d (0 .. %d)", b, (int)item_start[b], kMaxRows);
    rec[b] = SolverItem{row0[k], (int)table_rows[k], (int)item_start[b], flags[k]};
    S = std::max(S, rec[b].start + rec[b].steps);
    any_noise |= (flags[k] & SOLVER_ITEM_NOISE) != 0;
    any_h2 |= (flags[k] & SOLVER_ITEM_HIST2) != 0;
  }
  if (item_corrections_fit(h, rec.data(), n_items, (int)rows)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (!h->coef_dev) HIPCHK(hipMalloc((void**)&h->coef_dev, (size_t)kMaxRows * NS2VC_NCOEF * sizeof(float)));
  if (h->items.reserve(h, (size_t)n_items, false)) return 1;
  HIPCHK(hipDeviceSynchronize());   // a previous loop may still be reading the table
  HIPCHK(hipMemcpy(h->coef_dev, coef_host, (size_t)rows * NS2VC_NCOEF * sizeof(float), hipMemcpyHostToDevice));
  if (h->items.send(rec.data(), (size_t)n_items, s)) return 1;
  const size_t nb = (size_t)n_items * sizeof(SolverItem);
  {      // the hand-off's table hash covers the rows and the records
    unsigned long long hsh = 1469598103934665603ull;
    const unsigned char* pb = reinterpret_cast<const unsigned char*>(coef_host);
    for (size_t i = 0; i < (size_t)rows * NS2VC_NCOEF * sizeof(float); ++i) { hsh ^= pb[i]; hsh *= 1099511628211ull; }
    pb = reinterpret_cast<const unsigned char*>(rec.data());
    for (size_t i = 0; i < nb; ++i) { hsh ^= pb[i]; hsh *= 1099511628211ull; }
    h->coef_hash = hsh;
  }
  // (which update runs, its noise arguments and its m_prev2 pointer are baked into the captured step graph)
  if (!h->items.on || any_noise != h->stochastic || any_h2 != h->hist2.on) drop_step_graph(h);
  h->items.on = true;
  h->items.n = n_items;
  h->items.rows = (int)rows;
  h->items.host = rec;
  h->steps = S;
  h->stochastic = any_noise;
  h->hist2.on = any_h2;
  h->temb_table_valid = false;
  h->next_step = -1;
  return 0;
}

// the m_{i-2} buffer of history-2 tables for the prepared shape
static int ensure_mprev2(ns2vc_unet* h) { return h->hist2.reserve(h, (size_t)h->B * h->T * h->CP, false); }

int ns2vc_sampler_set_seeds(ns2vc_unet* h, const uint64_t* seeds_b, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!seeds_b) return fail("null seeds");
  hipStream_t s = (hipStream_t)stream;
  const int B = h->loop_items();      // (guided: n seeds, both halves get the same noise)
  if (h->seeds.reserve(h, (size_t)B, true) || h->seeds.send(reinterpret_cast<const unsigned long long*>(seeds_b), (size_t)B, s)) return 1;
  h->seeds.set = true;
  return 0;
}

static int guidance_onoff(ns2vc_unet* h, bool on, int n) {
  if (on != h->guide.on) {
    drop_step_graph(h);      // (the step graph bakes in which update runs)
    h->seeds.set = false;    // (B seeds are not the n seeds of a guided loop, nor the other way round)
    h->slots.on = false;     // (nor a slot loop: open it again)
    h->next_step = -1;       // (nor does a loop in progress survive the change)
    h->hold.on = false;      // (nor known frames: their mask covered the other item count)
    h->hold.n = 0;
    h->shold.drop(h);      // (nor a slot loop's: its state covered the other item count)
  }
  h->guide.on = on;
  h->guide.n = on ? n : 0;
  return 0;
}

int ns2vc_sampler_set_guidance(ns2vc_unet* h, const float* scale_host, int n, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!scale_host) return guidance_onoff(h, false, 0);
  if (n <= 0 || h->B != 2 * n) return fail("guidance for n = %d items needs an engine prepared for B = 2n (B = %d)", n, h->B);
  for (int b = 0; b < n; ++b)
    if (!std::isfinite(scale_host[b])) return fail("guidance scale[%d] is not finite", b);
  hipStream_t s = (hipStream_t)stream;
  if (h->guide.reserve(h, (size_t)n, true) || h->guide.send(scale_host, (size_t)n, s)) return 1;
  return guidance_onoff(h, true, n);
}

// the threshold buffer of the dynamic thresholding: one float per batch item
static int ensure_thr(ns2vc_unet* h) { return h->x0c.thr.reserve(h, (size_t)h->B, true); }
static int x0_correction_set(ns2vc_unet* h, int mode, float ratio, float max_val) {
  // the step graph bakes in what the active mode passes to its launches: mode 1 the ratio (quantile launch) and max_val (update), mode 2 max_val alone,
  // mode 0 nothing -- a change of a value no launch takes recaptures nothing
  const bool same = mode == h->x0c.mode && (mode == 0 || (max_val == h->x0c.max_val && (mode == 2 || ratio == h->x0c.ratio)));
  if (!same) drop_step_graph(h);
  h->x0c.mode = mode; h->x0c.ratio = ratio; h->x0c.max_val = max_val;
  if (mode == 1 && h->B > 0 && ensure_thr(h)) return 1;
  return 0;
}

int ns2vc_sampler_set_x0_correction(ns2vc_unet* h, int mode, float ratio, float max_val) {
  if (check_ready(h, false)) return 1;
  if (mode < 0 || mode > 2) return fail("x0 correction mode %d: 0 (off), 1 (dynamic thresholding) or 2 (clamp)", mode);
  if (!(ratio >= 0.f && ratio <= 1.f)) return fail("dynamic thresholding ratio %g outside [0, 1]", (double)ratio);
  if (!(std::isfinite(max_val) && max_val > 0.f)) return fail("thresholding max_val %g must be finite and > 0", (double)max_val);
  if (mode && h->hold.on)
    return fail("known frames are held (ns2vc_sampler_set_known): an x0 correction would rescale them; switch the hold off (NULL, NULL) before "
                "ns2vc_sampler_set_x0_correction(mode %d)", mode);
  if (mode && h->shold.on && h->in_slot_loop())
    return fail("the slot loop holds known frames (ns2vc_sampler_open_known): an x0 correction would rescale them; open the loop without them before "
                "ns2vc_sampler_set_x0_correction(mode %d)", mode);
  if (mode && h->x0c.items.on)
    return fail("the per-item x0 correction is on (ns2vc_sampler_set_x0_correction_items): switch it off (NULL arrays) before the loop-wide "
                "ns2vc_sampler_set_x0_correction(mode %d)", mode);
  return x0_correction_set(h, mode, ratio, max_val);
}

// The per-item form: one record per loop item, read by the step's two launches from device memory.  On / off, a new buffer and the presence of the
// quantile launch recapture; new values replay.
int ns2vc_sampler_set_x0_correction_items(ns2vc_unet* h, const int32_t* mode_host, const float* ratio_host, const float* max_val_host, int n, void* stream) {
  if (check_ready(h, true)) return 1;
  auto& ic = h->x0c.items;
  if (!mode_host && !ratio_host && !max_val_host) {      // off
    if (ic.on) drop_step_graph(h);
    ic.on = false; ic.quant = false; ic.n = 0;
    return 0;
  }
  if (!mode_host || !ratio_host || !max_val_host) return fail("per-item x0 correction: mode, ratio and max_val are given together (all NULL = off)");
  if (h->x0c.mode)
    return fail("the loop-wide x0 correction is on (ns2vc_sampler_set_x0_correction mode %d): switch it off (mode 0) before "
                "ns2vc_sampler_set_x0_correction_items", h->x0c.mode);
  if (h->hold.on)
    return fail("known frames are held (ns2vc_sampler_set_known): an x0 correction would rescale them; switch the hold off (NULL, NULL) before "
                "ns2vc_sampler_set_x0_correction_items");
  if (h->shold.on && h->in_slot_loop())
    return fail("the slot loop holds known frames (ns2vc_sampler_open_known): an x0 correction would rescale them; open the loop without them before "
                "ns2vc_sampler_set_x0_correction_items");
  if (n != h->loop_items())
    return fail("per-item x0 correction for %d items, the loop takes %d (the prepared batch; n under guidance: set the guidance first)", n, h->loop_items());
  std::vector<ItemCorrect> rec;
  bool dyn = false;
  if (item_corrections_from(mode_host, ratio_host, max_val_host, n, rec, dyn)) return 1;
  const bool slot_loop = h->in_slot_loop();
  // a slot loop's admitted items are checked here (nothing looks at them again; an idle slot has no flags); closed schedules are checked when they
  // load and when the loop begins, so the table and the schedules of a new batch may arrive in either order
  if (slot_loop && (int)h->slots.rec.size() == n) {
    std::vector<SolverItem> cur = h->slots.rec;      // (a resumed request's start lies in the past, below 0 after a rebase: ns2vc_sampler_resume)
    for (SolverItem& r : cur) r.start = std::max(r.start, 0);
    if (solver_items_fit("slot", cur.data(), nullptr, n, h->items.rows, nullptr, nullptr, nullptr, 0, rec.data())) return 1;
  }
  if (ic.reserve(h, (size_t)n, false) || ensure_thr(h) || ic.send(rec.data(), (size_t)n, (hipStream_t)stream)) return 1;
  const bool quant = dyn || slot_loop;      // (a slot loop always has the launch: its admissions bring records the host cannot foresee)
  if (!ic.on || quant != ic.quant) drop_step_graph(h);
  ic.on = true; ic.quant = quant; ic.n = n;
  ic.host = rec;
  return 0;
}

// Known frames: the caller's latent on the masked frames of every loop item, written over x0 at every step.  On / off recaptures;
// new values and new masks are copies into buffers that hold the whole prepared shape, so they replay.
int ns2vc_sampler_set_known(ns2vc_unet* h, const float* known_nct, const uint8_t* mask_nt, int n, void* stream) {
  if (check_ready(h, true)) return 1;
  auto& k = h->hold;
  if (!known_nct && !mask_nt) {      // off
    if (k.on) drop_step_graph(h);
    k.on = false; k.n = 0; k.last.clear();
    return 0;
  }
  if (!known_nct || !mask_nt) return fail("known frames: the latent and the mask are given together (both NULL = off)");
  if (n != h->loop_items())
    return fail("known frames for %d items, the loop takes %d (the prepared batch; n under guidance: set the guidance first)", n, h->loop_items());
  if (h->x0c.mode || h->x0c.items.on)
    return fail("an x0 correction is on (ns2vc_sampler_set_x0_correction%s): it would rescale the known frames; switch it off before ns2vc_sampler_set_known",
                h->x0c.mode ? "" : "_items");
  if (h->in_slot_loop()) return fail("a slot loop is open (ns2vc_sampler_open): known frames run in closed loops only");
  const size_t rows = (size_t)n * h->T;
  if (rows > (size_t)0x7fffffff - HOLD_LIST_HEAD) return fail("known frames: %zu rows exceed the 32-bit row list", rows);
  std::vector<int> list;
  std::vector<int32_t> last;
  if (hold_list_from_mask(mask_nt, n, h->T, h->lens.masked ? h->lens.applied.data() : nullptr, list, last)) return 1;
  hipStream_t s = (hipStream_t)stream;
  if (k.known.reserve(h, rows * h->CP, false) || k.rows.reserve(h, (size_t)HOLD_LIST_HEAD + rows, true)) return 1;
  HIPCHK(launch_nct_to_btc(known_nct, h->cfg.latent_channels, h->T, n, k.known.dev, nullptr, PREC_F32, h->CP, h->CP, s));
  if (k.rows.send(list.data(), list.size(), s)) return 1;
  if (!k.on) drop_step_graph(h);
  k.on = true; k.n = n; k.last = last;
  return 0;
}

// one evaluation + solver update
static int run_step(ns2vc_unet* h, hipStream_t s, bool capturing = false) {
  GemmArgs g;
  const bool fold = solver_in_conv_out(h, g);
  const size_t last = fold ? (size_t)h->conv_out_idx : h->fwd_ops.size();
  size_t first = 0;
  // r6: under capture the timestep-embedding branch becomes a parallel branch of the graph (fork after the statistics clear, which advances the step counter
  // the branch reads; join in front of the first launch that reads the scale / shift rows).  Eager loops keep one stream: same launches, same results.
  if (capturing && temb_forks(h, last)) {
    if (!h->tfork.side_stream) HIPCHK(hipStreamCreateWithFlags(&h->tfork.side_stream, hipStreamNonBlocking));
    if (!h->tfork.ev_fork) HIPCHK(hipEventCreateWithFlags(&h->tfork.ev_fork, hipEventDisableTiming));
    if (!h->tfork.ev_join) HIPCHK(hipEventCreateWithFlags(&h->tfork.ev_join, hipEventDisableTiming));
    if (run_ops(h->fwd_ops, s, 0, (size_t)h->tfork.begin)) return 1;
    HIPCHK(hipEventRecord(h->tfork.ev_fork, s));
    HIPCHK(hipStreamWaitEvent(h->tfork.side_stream, h->tfork.ev_fork, 0));
    if (run_ops(h->fwd_ops, h->tfork.side_stream, (size_t)h->tfork.begin, (size_t)h->tfork.end)) return 1;
    HIPCHK(hipEventRecord(h->tfork.ev_join, h->tfork.side_stream));
    if (run_ops(h->fwd_ops, s, (size_t)h->tfork.end, (size_t)h->tfork.join)) return 1;
    HIPCHK(hipStreamWaitEvent(s, h->tfork.ev_join, 0));
    first = (size_t)h->tfork.join;
  }
  if (run_ops(h->fwd_ops, s, first, last)) return 1;
  if (fold) {
    HIPCHK(launch_gemm(g, h->conv_out_prec, s));
    return 0;
  }
  if (h->items.on && h->items.n != h->loop_items())
    return fail("per-item schedules for %d items, the loop has %d (load them again)", h->items.n, h->loop_items());
  const auto& ic = h->x0c.items;
  if (ic.on && !h->items.on) return fail("the per-item x0 correction runs on per-item records: load them (ns2vc_sampler_load_items) or open a slot loop");
  if (ic.on && ic.n != h->loop_items()) return fail("the per-item x0 correction holds %d records, the loop has %d items (set it again)", ic.n, h->loop_items());
  if (h->hold.on) {      // the known frames go over the x0 the plan's last launch wrote, in front of everything that reads it
    if (h->hold.n != h->loop_items()) return fail("known frames for %d items, the loop has %d (set them again)", h->hold.n, h->loop_items());
    HIPCHK(launch_hold_x0(h->x0, h->hold.known.dev, h->hold.rows.dev, h->hold.n * h->T, h->CP, h->cfg.latent_channels, h->guide.on ? 2 : 1, s));
  }
  if (h->shold.on) {     // a slot loop's known frames: the same place, the held rows by the per-slot byte mask
    if ((int)h->shold.last.size() != h->loop_items()) return fail("the slot loop's known frames cover %d slots, the loop has %d (open it again)", (int)h->shold.last.size(), h->loop_items());
    HIPCHK(launch_hold_slots(h->x0, h->shold.known.dev, h->shold.mask.dev, h->loop_items() * h->T, h->CP, h->cfg.latent_channels, h->guide.on ? 2 : 1, s));
  }
  SolverStep st;
  st.coef = h->coef_dev; st.step_ptr = h->step_dev; st.ncoef = NS2VC_NCOEF;
  st.x0 = h->x0; st.xe = h->xe; st.xe_op = h->xe_op; st.prec = h->prec; st.xbar = h->xbar; st.d1 = h->d1; st.mprev = h->mprev;
  if (h->hist2.on) st.mprev2 = h->hist2.dev;
  st.n = (size_t)h->loop_items() * h->T * h->CP;      // (guided: the elements of one half)
  st.T = h->T; st.ld = h->CP; st.nc = h->cfg.latent_channels; st.split = h->pair_off();
  if (h->lens.masked) st.lens = h->lens.dev;      // the item's valid frames (level-0 lengths = the first B entries): what the noise and the quantile cover
  if (h->guide.on) st.scale = h->guide.dev;
  if (h->stochastic) st.seeds = h->seeds.dev;
  if (h->items.on) { st.items = h->items.dev; st.n_items = h->items.n; }
  if (ic.on) { st.item_correct = ic.dev; st.quant = ic.quant; }
  else { st.mode = h->x0c.mode; st.ratio = h->x0c.ratio; st.max_val = h->x0c.max_val; }      // (not with a stochastic table: ns2vc_sampler_begin refuses the pair)
  st.thr = h->x0c.thr.dev;
  HIPCHK(launch_solver_step(st, s));
  return 0;
}

// The loop in three parts, so that a caller can hand the solver state to a second engine in mid-loop (mixed precision:
// ns2vc_sampler_handoff): begin = state from x_T, steps = the next n evaluations + updates, end = layout change back.
int ns2vc_sampler_begin(ns2vc_unet* h, const float* x_T_bct, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!x_T_bct) return fail("null tensor");
  h->shold.drop(h);      // (a closed loop never runs a slot loop's hold launch)
  if (h->slots.on) {      // begin takes whole batches: it leaves slot mode, whose table rows and records belong to the slots' items
    h->slots.on = false; h->steps = 0; h->next_step = -1;
    return fail("the engine ran a slot loop (ns2vc_sampler_open), which this call has ended: load a table (ns2vc_sampler_load / _load_items) before ns2vc_sampler_begin");
  }
  if (!h->coef_dev || h->steps <= 0) return fail("no solver table loaded (call ns2vc_sampler_load)");
  if (h->items.on && h->items.n != h->loop_items())
    return fail("per-item schedules for %d items, the loop takes %d: load them again (ns2vc_sampler_load_items)", h->items.n, h->loop_items());
  if (h->stochastic && !h->seeds.set) return fail("the loaded solver table adds noise: set per-item seeds first (ns2vc_sampler_set_seeds)");
  if (h->stochastic && h->x0c.mode)
    return fail("the x0 correction (mode %d) does not apply to a stochastic table (ddpm, ddim with eta > 0): the reference's discrete samplers have none; "
                "turn it off (ns2vc_sampler_set_x0_correction) or load a noise-free table", h->x0c.mode);
  if (h->x0c.mode == 1 && ensure_thr(h)) return 1;
  if (h->x0c.items.on) {
    if (!h->items.on)
      return fail("the per-item x0 correction (ns2vc_sampler_set_x0_correction_items) reads per-item records and this is a shared table (ns2vc_sampler_load): "
                  "load the schedules with ns2vc_sampler_load_items, or switch the table off");
    if (item_corrections_fit(h, h->items.host.data(), h->items.n, h->items.rows)) return 1;
    if (ensure_thr(h)) return 1;
  }
  if (h->hold.on) {
    if (h->hold.n != h->loop_items())
      return fail("known frames for %d items, the loop takes %d: set them again (ns2vc_sampler_set_known)", h->hold.n, h->loop_items());
    if (h->x0c.mode || h->x0c.items.on) return fail("known frames do not run with an x0 correction: it would rescale them");
    if (h->lens.masked)      // (lengths set after the mask)
      for (int b = 0; b < h->hold.n; ++b)
        if (h->hold.last[(size_t)b] >= h->lens.applied[(size_t)b])
          return fail("known frame %d of item %d lies at or past its length %d: set the known frames after the lengths", (int)h->hold.last[(size_t)b], b,
                      (int)h->lens.applied[(size_t)b]);
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)h->B * h->T * h->CP;
  if (h->guide.on) {      // n items of x_T into the unconditional half, the same point into the conditional half
    const int gn = h->guide.n;
    if (h->lens.masked)
      for (int b = 0; b < gn; ++b)
        if (h->lens.applied[b] != h->lens.applied[b + gn])
          return fail("guided loop: lengths[%d] = %d and lengths[%d] = %d differ (the two halves hold the same latents)", b, (int)h->lens.applied[b], b + gn,
                      (int)h->lens.applied[b + gn]);
    const size_t nh = n / 2, ohb = nh / h->CP * h->pair_width() * operand_bytes(h->prec);
    if (load_state(h, x_T_bct, s, gn)) return 1;
    HIPCHK(launch_copy16(h->xe, h->xe + nh, nh * sizeof(float), s));
    HIPCHK(launch_copy16(h->xe_op, static_cast<char*>(h->xe_op) + ohb, ohb, s));
    HIPCHK(launch_copy16(h->xe, h->xbar, nh * sizeof(float), s));
    HIPCHK(launch_zero(h->xbar + nh, nh * sizeof(float), s));      // (the histories live in the first half; the second stays zero)
  } else {
    if (load_state(h, x_T_bct, s)) return 1;  // (masked: x_T is zero past every item's end; the solver update keeps it so -- its noise term skips those rows)
    HIPCHK(launch_copy16(h->xe, h->xbar, n * sizeof(float), s));
  }
  HIPCHK(launch_zero(h->d1, n * sizeof(float), s));
  HIPCHK(launch_zero(h->mprev, n * sizeof(float), s));
  if (h->hist2.on) {
    if (ensure_mprev2(h)) return 1;
    HIPCHK(launch_zero(h->hist2.dev, n * sizeof(float), s));
  }
  HIPCHK(launch_fill_i32(h->step_dev, -1, s));      // the first launch of every step advances it (gn_stats.clear)
  h->next_step = 0;
  return 0;
}

int ns2vc_sampler_steps(ns2vc_unet* h, int n_steps, int use_graph, void* stream) {
  if (check_ready(h, true)) return 1;
  const bool slot_loop = h->in_slot_loop();      // (no table length bounds a slot loop: S follows the admissions, idle steps are legal)
  if (!h->coef_dev || (h->steps <= 0 && !slot_loop)) return fail("no solver table loaded (call ns2vc_sampler_load)");
  if (h->next_step < 0) return fail("no sampling loop in progress (call ns2vc_sampler_begin or ns2vc_sampler_handoff)");
  if (h->hist2.on && !h->hist2.dev) return fail("history-2 table without its m_prev2 buffer (begin the loop after loading the table)");
  if (h->stochastic && h->x0c.mode) return fail("the x0 correction does not apply to a stochastic table");
  if (h->x0c.mode == 1 && ensure_thr(h)) return 1;
  if (h->x0c.items.on && (!h->items.on || ensure_thr(h)))
    return h->items.on ? 1 : fail("the per-item x0 correction reads per-item records: load them with ns2vc_sampler_load_items");
  if (slot_loop) {
    if (n_steps < 0 || n_steps > SOLVER_ITEM_NEVER - 1 - h->next_step)
      return fail("%d steps from loop step %d pass the end of the 32-bit step counter: drain the slots and call ns2vc_sampler_rebase", n_steps, h->next_step);
  } else if (n_steps < 0 || h->next_step + n_steps > h->steps) return fail("steps %d..%d outside the loaded table of %d", h->next_step, h->next_step + n_steps, h->steps);
  hipStream_t s = (hipStream_t)stream;
  const auto& c = h->cfg;
  h->use_step_table = true;
  if (!h->temb_table_valid) {      // new table or new weights: timestep MLP of every table row (column 0 = t), no prompt term
    const int E = c.block_out_channels[0] * 4;
    if (!h->temb_table) HIPCHK(hipMalloc((void**)&h->temb_table, (size_t)1024 * E * sizeof(float)));
    HIPCHK(launch_time_embed(h->coef_dev, NS2VC_NCOEF, nullptr, 0, h->t_w1t, h->t_b1, h->t_w2t, h->t_b2, nullptr, h->temb_table, nullptr,
                             h->prec, h->items.on ? h->items.rows : h->steps, c.block_out_channels[0], E, s));      // (per-item schedules: the rows of all distinct tables)
    h->temb_table_valid = true;
  }
  if (use_graph && !h->step_graph && n_steps > 0) {
    if (!h->cap_stream) HIPCHK(hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    HIPCHK(hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal));
    const int rc = run_step(h, h->cap_stream, true);
    hipError_t e = hipStreamEndCapture(h->cap_stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
    if (e != hipSuccess) return fail("hipStreamEndCapture: %s", hipGetErrorString(e));
    e = hipGraphInstantiate(&h->step_graph, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    if (e != hipSuccess) { h->step_graph = nullptr; return fail("hipGraphInstantiate: %s", hipGetErrorString(e)); }
    ++h->graph_captures;
  }
  for (int i = 0; i < n_steps; ++i) {
    if (use_graph) HIPCHK(hipGraphLaunch(h->step_graph, s));
    else if (run_step(h, s)) return 1;
  }
  h->next_step += n_steps;
  return 0;
}

// Solver state of `src` (x_e, x_bar, d1, m_prev, m_prev2 of history-2 tables, loop position) -> `dst`, which continues the SAME table from there: the
// engines may differ in precision (the state is fp32 in every mode; dst's operand copy of x_e is rebuilt in its own type).
// Both must be prepared for the same (B, T) and hold the same solver table and condition.  The guidance of `src` (on / off, n, the scales)
// and its x0 correction (mode, ratio, max_val) become those of `dst`; a guided loop's histories live in the first halves, and x_e and its operand copy in both.
int ns2vc_sampler_handoff(ns2vc_unet* dst, ns2vc_unet* src, void* stream) {
  if (check_ready(dst, true) || check_ready(src, true)) return 1;
  if (dst == src) return fail("handoff to the same engine");
  if (dst->B != src->B || dst->T != src->T || dst->CP != src->CP) return fail("handoff between different shapes");
  if (dst->device != src->device) return fail("handoff between engines on different devices");
  if (src->next_step < 0) return fail("source engine has no sampling loop in progress");
  if (src->in_slot_loop() || dst->in_slot_loop())
    return fail("a slot loop (ns2vc_sampler_open) cannot be handed off: its slots stand at different rows of different tables; run requests that need an fp32 tail on an fp32 engine");
  if (!dst->coef_dev || dst->steps != src->steps) return fail("destination engine must hold the same solver table (%d vs %d steps)", dst->steps, src->steps);
  if (dst->items.on != src->items.on || (src->items.on && dst->items.n != src->items.n))
    return fail("destination engine must hold the same per-item schedules (ns2vc_sampler_load_items on both, or on neither)");
  if (dst->hold.on != src->hold.on || (src->hold.on && dst->hold.n != src->hold.n))
    return fail("the two engines disagree on known frames (ns2vc_sampler_set_known): set the same latent and mask on both, or on neither");
  if (dst->coef_hash != src->coef_hash) return fail("destination engine holds a DIFFERENT solver table with the same number of steps (solver / order / betas differ)");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)src->B * src->T * src->CP;
  const size_t nh = (size_t)src->loop_items() * src->T * src->CP;      // the histories' extent (guided: the first half)
  if (src->guide.on) {
    if (dst->guide.reserve(dst, (size_t)src->guide.n, true)) return 1;
    HIPCHK(launch_copy16(src->guide.dev, dst->guide.dev, dst->guide.rounded((size_t)src->guide.n) * sizeof(float), s));
  }
  guidance_onoff(dst, src->guide.on, src->guide.n);
  {      // (the tail corrects as the head does: the loop-wide setting, or the per-item table and its records)
    const auto& sc = src->x0c.items;
    auto& dc = dst->x0c.items;
    if (!sc.on) {
      if (dc.on) drop_step_graph(dst);
      dc.on = false; dc.quant = false; dc.n = 0;
    }
    if (x0_correction_set(dst, src->x0c.mode, src->x0c.ratio, src->x0c.max_val)) return 1;
    if (sc.on) {
      if (dc.reserve(dst, (size_t)sc.n, false) || ensure_thr(dst)) return 1;
      HIPCHK(launch_copy16(sc.dev, dc.dev, (size_t)sc.n * sizeof(ItemCorrect), s));
      if (!dc.on || dc.quant != sc.quant) drop_step_graph(dst);
      dc.on = true; dc.quant = sc.quant; dc.n = sc.n; dc.host = sc.host;
    }
  }
  HIPCHK(launch_copy16(src->xe, dst->xe, n * sizeof(float), s));
  HIPCHK(launch_copy16(src->xbar, dst->xbar, nh * sizeof(float), s));
  HIPCHK(launch_copy16(src->d1, dst->d1, nh * sizeof(float), s));
  HIPCHK(launch_copy16(src->mprev, dst->mprev, nh * sizeof(float), s));
  if (src->hist2.on) {          // (same table hash: dst->hist2.on too)
    if (ensure_mprev2(dst)) return 1;
    HIPCHK(launch_copy16(src->hist2.dev, dst->hist2.dev, nh * sizeof(float), s));
  }
  HIPCHK(launch_cast_op(dst->xe, n, dst->xe_op, dst->prec, s, dst->pair_off()));
  if (src->seeds.set) {      // the tail continues the same noise stream
    const int ns = src->loop_items();
    if (dst->seeds.reserve(dst, (size_t)ns, true)) return 1;
    HIPCHK(launch_copy16(src->seeds.dev, dst->seeds.dev, dst->seeds.rounded((size_t)ns) * sizeof(unsigned long long), s));
    dst->seeds.set = true;
  }
  HIPCHK(launch_fill_i32(dst->step_dev, src->next_step - 1, s));
  dst->next_step = src->next_step;
  src->next_step = -1;
  return 0;
}

int ns2vc_sampler_peek(ns2vc_unet* h, float* x_out_bct, void* stream) {
  if (check_ready(h, true)) return 1;
  if (!x_out_bct) return fail("null tensor");
  if (h->next_step < 0) return fail("no sampling loop in progress");
  HIPCHK(launch_btc_to_nct(h->xe, h->CP, h->cfg.latent_channels, h->T, h->loop_items(), x_out_bct, (hipStream_t)stream));      // (guided: the n items)
  return 0;
}

int ns2vc_sampler_end(ns2vc_unet* h, float* x_out_bct, void* stream) {
  if (ns2vc_sampler_peek(h, x_out_bct, stream)) return 1;
  h->next_step = -1;
  h->slots.on = false;
  h->shold.last.clear();      // (a slot loop's known frames end with it; the form stays baked until the next loop is opened or a table loaded)
  return 0;
}

int ns2vc_sampler_run(ns2vc_unet* h, float* x_inout_bct, int use_graph, void* stream) {
  if (ns2vc_sampler_begin(h, x_inout_bct, stream)) return 1;
  if (ns2vc_sampler_steps(h, h->steps, use_graph, stream)) return 1;
  return ns2vc_sampler_end(h, x_inout_bct, stream);
}

}  // extern "C"

// ---- slot loop ----------------------------------------------------------------------------------------------------------------
static const int kSlotRows = 1024;      // the coefficient table's fixed capacity (ns2vc_sampler_load's)

int ns2vc::stage_slot_list(ns2vc_unet* h, int n, const int32_t* slots, int nslots, const SolverItem* rec, hipStream_t s, const int** slots_dev,
                           const SolverItem** rec_dev, const void* extra, size_t extra_bytes, void* extra_dev) {
  if (!slots || n <= 0 || n > nslots) return fail("a slot list needs 1 .. %d entries, got %d", nslots, n);
  std::vector<char> seen((size_t)nslots, 0);
  for (int k = 0; k < n; ++k) {
    if (slots[k] < 0 || slots[k] >= nslots) return fail("slots[%d] = %d outside [0, %d)", k, (int)slots[k], nslots);
    if (seen[slots[k]]) return fail("slot %d is listed twice", (int)slots[k]);
    seen[slots[k]] = 1;
  }
  auto& sl = h->slots;
  if (!sl.list_dev || sl.cap < nslots) {      // (the kernels take the pointer as a launch argument: no captured graph holds it)
    if (sl.list_dev) { HIPCHK(hipStreamSynchronize(s)); HIPCHK(hipFree(sl.list_dev)); sl.list_dev = nullptr; sl.cap = 0; }
    HIPCHK(hipMalloc((void**)&sl.list_dev, (size_t)nslots * 5 * sizeof(int)));
    sl.cap = nslots;
  }
  Staged& st = sl.ring[sl.ring_next];
  sl.ring_next = (sl.ring_next + 1) % ns2vc_unet::SlotLoop::kRing;
  const size_t lb = (size_t)n * sizeof(int), rb = rec ? (size_t)n * sizeof(SolverItem) : 0;
  if (st.reserve(lb + rb + extra_bytes)) return 1;
  memcpy(st.buf, slots, lb);
  if (rec) memcpy(static_cast<char*>(st.buf) + lb, rec, rb);
  if (extra_bytes) {
    memcpy(static_cast<char*>(st.buf) + lb + rb, extra, extra_bytes);
    HIPCHK(hipMemcpyAsync(extra_dev, static_cast<char*>(st.buf) + lb + rb, extra_bytes, hipMemcpyHostToDevice, s));
  }
  HIPCHK(hipMemcpyAsync(sl.list_dev, st.buf, lb, hipMemcpyHostToDevice, s));
  SolverItem* rd = reinterpret_cast<SolverItem*>(sl.list_dev + sl.cap);
  if (rec) HIPCHK(hipMemcpyAsync(rd, static_cast<char*>(st.buf) + lb, rb, hipMemcpyHostToDevice, s));
  if (st.record(s)) return 1;
  *slots_dev = sl.list_dev;
  if (rec_dev) *rec_dev = rec ? rd : nullptr;
  return 0;
}

static int need_slot_loop(ns2vc_unet* h) {
  if (check_ready(h, true)) return 1;
  if (!h->in_slot_loop()) return fail("no slot loop is open (call ns2vc_sampler_open)");
  return 0;
}

extern "C" {

// ns2vc_sampler_open and ns2vc_sampler_open_known (known != 0: the per-slot known-frame form)
static int sampler_open(ns2vc_unet* h, int history2, int noise, int known, void* stream) {
  if (check_ready(h, true)) return 1;
  hipStream_t s = (hipStream_t)stream;
  auto& sl = h->slots;
  const int n = h->loop_items();
  const bool h2 = history2 != 0, nz = noise != 0;
  if (h->hold.on) return fail("known frames are held (ns2vc_sampler_set_known): a slot loop does not run with them; switch the hold off (NULL, NULL) first");
  if (h->fuse_solver) return fail("option fuse_solver folds the shared-table update into conv_out: a slot loop does not run with it (set it to 0 and prepare again)");
  if (nz && h->x0c.mode)
    return fail("a slot loop with stochastic items does not run with the x0 correction (mode %d): turn one of them off before ns2vc_sampler_open", h->x0c.mode);
  if (h->guide.on && h->lens.masked)
    for (int b = 0; b < n; ++b)
      if (h->lens.applied[b] != h->lens.applied[b + n]) return fail("guided slot loop: lengths[%d] and lengths[%d] differ", b, b + n);
  if (h->in_slot_loop() && sl.any_busy()) return fail("the slot loop is open and has busy slots: take them before opening again");
  if (known && (h->x0c.mode || h->x0c.items.on))
    return fail("an x0 correction is on (ns2vc_sampler_set_x0_correction%s): it would rescale the known frames; switch it off before ns2vc_sampler_open_known",
                h->x0c.mode ? "" : "_items");
  const size_t tb = (size_t)kSlotRows * NS2VC_NCOEF * sizeof(float);
  if (!h->coef_dev) HIPCHK(hipMalloc((void**)&h->coef_dev, tb));
  if (h->items.reserve(h, (size_t)n, false)) return 1;
  if (!sl.list_dev || sl.cap < h->B) {      // the slot lists of every later call fit (B covers both halves of a guided engine): no call in mid-loop grows it
    if (sl.list_dev) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(sl.list_dev)); sl.list_dev = nullptr; sl.cap = 0; }
    HIPCHK(hipMalloc((void**)&sl.list_dev, (size_t)h->B * 5 * sizeof(int)));
    sl.cap = h->B;
  }
  if (h2 && ensure_mprev2(h)) return 1;
  if (nz && h->seeds.reserve(h, (size_t)n, true)) return 1;
  auto& kh = h->shold;
  if (known) {      // the per-slot state for the whole prepared shape, and staging room for the largest mask: no later call of the loop allocates
    const size_t rows = (size_t)n * h->T;
    if (rows > (size_t)0x7fffffff) return fail("known frames: %zu rows exceed the 32-bit row index", rows);
    if (kh.known.reserve(h, rows * h->CP, true) || kh.mask.reserve(h, rows, true) || kh.mask_in.reserve(h, rows, true)) return 1;
    for (Staged& st : sl.ring)
      if (st.reserve((size_t)n * (sizeof(int) + sizeof(SolverItem)) + rows)) return 1;
  }
  if ((known != 0) != kh.on) drop_step_graph(h);      // (the hold launch is part of the captured step or it is not)
  if (h->x0c.mode == 1 && ensure_thr(h)) return 1;
  if (h->x0c.items.on) {      // the per-item x0 correction is baked in beside history 2 and noise: every slot off until its admission brings a record
    auto& ic = h->x0c.items;
    if (ic.n != n) return fail("the per-item x0 correction holds %d records, the slot loop has %d slots: set it again (ns2vc_sampler_set_x0_correction_items)", ic.n, n);
    if (ensure_thr(h)) return 1;
    if (!ic.quant) drop_step_graph(h);      // (a slot loop always runs the quantile launch: the host cannot foresee its admissions)
    ic.quant = true;
  }
  // (which update runs, its noise arguments and its m_prev2 pointer are baked into the captured step graph)
  if (!h->items.on || nz != h->stochastic || h2 != h->hist2.on) drop_step_graph(h);
  // every slot idle, on finite data: a zero table (model time 0 in every row), zero state, zero condition, hoisted tensors rebuilt from it
  const size_t ne = (size_t)h->B * h->T * h->CP;
  HIPCHK(launch_zero(h->coef_dev, tb, s));
  HIPCHK(launch_zero(h->xe, ne * sizeof(float), s));
  HIPCHK(launch_zero(h->xe_op, ne / h->CP * h->pair_width() * operand_bytes(h->prec), s));
  HIPCHK(launch_zero(h->xbar, ne * sizeof(float), s));
  HIPCHK(launch_zero(h->d1, ne * sizeof(float), s));
  HIPCHK(launch_zero(h->mprev, ne * sizeof(float), s));
  if (h2) HIPCHK(launch_zero(h->hist2.dev, ne * sizeof(float), s));
  {
    const auto& c = h->cfg;
    const size_t rows = (size_t)h->B * h->T;
    HIPCHK(launch_zero(h->content_op, rows * c.content_channels * (h->prec != PREC_F32 ? 2 : 1) * operand_bytes(h->prec), s));
    if (h->content_f32) HIPCHK(launch_zero(h->content_f32, rows * c.content_channels * sizeof(float), s));
    HIPCHK(launch_zero(h->prompt, (size_t)h->B * h->Lp * c.cross_attention_dim * sizeof(float), s));
    if (run_ops(h->cond_ops, s)) return 1;
    const int E = c.block_out_channels[0] * 4;
    if (!h->temb_table) HIPCHK(hipMalloc((void**)&h->temb_table, (size_t)kSlotRows * E * sizeof(float)));
    HIPCHK(launch_time_embed(h->coef_dev, NS2VC_NCOEF, nullptr, 0, h->t_w1t, h->t_b1, h->t_w2t, h->t_b2, nullptr, h->temb_table, nullptr, h->prec, kSlotRows,
                             c.block_out_channels[0], E, s));
    h->temb_table_valid = true;
  }
  sl.rec.assign((size_t)n, solver_item_idle());
  h->items.host = sl.rec;
  sl.busy.assign((size_t)n, 0);
  sl.coef.assign((size_t)kSlotRows * NS2VC_NCOEF, 0.f);
  if (h->items.send(sl.rec.data(), (size_t)n, s)) return 1;
  if (nz) h->seeds.set = true;      // (the buffer holds finite seeds; ns2vc_sampler_set_seeds gives the slots theirs)
  h->items.on = true;
  h->items.n = n;
  h->items.rows = kSlotRows;
  h->stochastic = nz;
  h->hist2.on = h2;
  h->steps = 0;
  h->coef_hash = 0;
  HIPCHK(launch_fill_i32(h->step_dev, -1, s));      // the first launch of every step advances it (gn_stats.clear)
  h->next_step = 0;
  sl.on = true;
  kh.on = known != 0;
  kh.last.clear();
  if (known) {      // no slot holds a frame
    HIPCHK(launch_zero(kh.mask.dev, (size_t)n * h->T, s));
    kh.last.assign((size_t)n, -1);
  }
  return 0;
}

int ns2vc_sampler_open(ns2vc_unet* h, int history2, int noise, void* stream) { return sampler_open(h, history2, noise, 0, stream); }
int ns2vc_sampler_open_known(ns2vc_unet* h, int history2, int noise, void* stream) { return sampler_open(h, history2, noise, 1, stream); }

// The known frames of the listed idle slots: the latent into the slots' known rows, the host mask through the staging ring into their
// mask bytes -- one launch; both NULL clears the listed slots.  A slot's frames last for one request: ns2vc_sampler_take clears them.
int ns2vc_sampler_set_known_items(ns2vc_unet* h, int n, const int32_t* slots, const float* known_nct, const uint8_t* mask_nt, void* stream) {
  if (need_slot_loop(h)) return 1;
  auto& kh = h->shold;
  const int ni = h->loop_items(), T = h->T;
  if (!kh.on) return fail("the slot loop was opened without known frames (ns2vc_sampler_open): open it with ns2vc_sampler_open_known");
  if ((known_nct != nullptr) != (mask_nt != nullptr)) return fail("known frames: the latent and the mask are given together (both NULL = clear the slots)");
  if ((int)kh.last.size() != ni || (int)h->slots.busy.size() != ni) return fail("the slot loop was opened for %d items, the loop has %d: open it again", (int)kh.last.size(), ni);
  if (!slots || n <= 0 || n > ni) return fail("a slot list needs 1 .. %d entries, got %d", ni, n);
  std::vector<int32_t> last((size_t)n, -1);
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    if (b < 0 || b >= ni) return fail("slots[%d] = %d outside [0, %d)", k, b, ni);
    if (h->slots.busy[b]) return fail("slot %d is busy: the known frames of a running request do not change (take it first)", b);
    if (!mask_nt) continue;
    const int L = h->lens.masked ? (int)h->lens.applied[(size_t)b] : T;
    for (int t = 0; t < T; ++t) {
      if (!mask_nt[(size_t)k * T + t]) continue;
      if (t >= L) return fail("known frame %d of slot %d lies at or past its length %d: set the lengths first", t, b, L);
      last[(size_t)k] = t;
    }
  }
  hipStream_t s = (hipStream_t)stream;
  const int* slots_dev = nullptr;
  if (stage_slot_list(h, n, slots, ni, nullptr, s, &slots_dev, nullptr, mask_nt, mask_nt ? (size_t)n * T : 0, kh.mask_in.dev)) return 1;
  HIPCHK(launch_known_items(known_nct, mask_nt ? kh.mask_in.dev : nullptr, h->cfg.latent_channels, T, n, slots_dev, ni, kh.known.dev, kh.mask.dev, h->CP, s));
  for (int k = 0; k < n; ++k) kh.last[(size_t)slots[k]] = last[(size_t)k];
  return 0;
}

// The 32-bit loop step must not bound a service's lifetime: with every slot idle (their records are "never active" at any step) the counter goes
// back to 0 -- one one-thread launch, no recapture; the table, the condition and the slots' state stay.
int ns2vc_sampler_rebase(ns2vc_unet* h, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (h->slots.any_busy()) return fail("the loop step is rebased on a drained loop only: take the busy slots first");
  HIPCHK(launch_fill_i32(h->step_dev, -1, (hipStream_t)stream));
  h->next_step = 0;
  h->steps = 0;
  return 0;
}

int ns2vc_sampler_write_rows(ns2vc_unet* h, int row0, int nrows, const float* coef_host, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (!coef_host || row0 < 0 || nrows <= 0 || row0 > kSlotRows - nrows) return fail("rows %d + %d outside the table of %d rows (its fixed capacity)", row0, nrows, kSlotRows);
  auto& sl = h->slots;
  for (size_t b = 0; b < sl.rec.size(); ++b) {      // a slot that has not finished reads its rows at every step still to come
    const SolverItem& r = sl.rec[b];
    if (sl.busy[b] && h->next_step < r.start + r.steps && r.row0 < row0 + nrows && row0 < r.row0 + r.steps)
      return fail("rows %d .. %d are in use: slot %d walks rows %d .. %d until loop step %d (now %d)", row0, row0 + nrows - 1, (int)b, r.row0,
                  r.row0 + r.steps - 1, r.start + r.steps, h->next_step);
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t nb = (size_t)nrows * NS2VC_NCOEF * sizeof(float);
  for (size_t i = 0; i < (size_t)nrows * NS2VC_NCOEF; ++i)
    if (!std::isfinite(coef_host[i])) return fail("table value %zu of the rows is not finite", i);
  Staged& st = sl.coef_ring[sl.coef_next];
  sl.coef_next = (sl.coef_next + 1) % ns2vc_unet::SlotLoop::kRing;
  if (st.reserve(nb)) return 1;
  memcpy(st.buf, coef_host, nb);
  memcpy(sl.coef.data() + (size_t)row0 * NS2VC_NCOEF, coef_host, nb);
  float* dst = h->coef_dev + (size_t)row0 * NS2VC_NCOEF;
  HIPCHK(hipMemcpyAsync(dst, st.buf, nb, hipMemcpyHostToDevice, s));
  if (st.record(s)) return 1;
  // the timestep MLP of these rows (column 0 = t): a row's embedding depends on that row alone, so the other rows keep their bits untouched
  const auto& c = h->cfg;
  const int E = c.block_out_channels[0] * 4;
  if (h->temb_table_valid)
    HIPCHK(launch_time_embed(dst, NS2VC_NCOEF, nullptr, 0, h->t_w1t, h->t_b1, h->t_w2t, h->t_b2, nullptr, h->temb_table + (size_t)row0 * E, nullptr, h->prec,
                             nrows, c.block_out_channels[0], E, s));      // (not valid: ns2vc_sampler_steps rebuilds the whole table)
  return 0;
}

int ns2vc_sampler_admit(ns2vc_unet* h, int n, const int32_t* slots, const float* x_T_nct, const int32_t* records, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (!x_T_nct || !records) return fail("null argument");
  auto& sl = h->slots;
  const int ni = h->loop_items();
  if (h->items.n != ni || (int)sl.rec.size() != ni) return fail("the slot loop was opened for %d items, the loop has %d: open it again", h->items.n, ni);
  if (h->stochastic && !h->seeds.set) return fail("the slot loop takes stochastic items: set per-item seeds first (ns2vc_sampler_set_seeds)");
  if (!slots || n <= 0 || n > ni) return fail("a slot list needs 1 .. %d entries, got %d", ni, n);
  static_assert(sizeof(SolverItem) == 4 * sizeof(int32_t), "records are four 32-bit words");
  const SolverItem* rec = reinterpret_cast<const SolverItem*>(records);
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    if (b < 0 || b >= ni) return fail("slots[%d] = %d outside [0, %d)", k, b, ni);
    if (sl.busy[b]) return fail("slot %d is busy (admitted at loop step %d for %d steps, not taken yet)", b, sl.rec[b].start, sl.rec[b].steps);
  }
  const auto& ic = h->x0c.items;
  if (solver_items_fit("slot", rec, slots, n, kSlotRows, sl.coef.data(),
                       h->hist2.on ? nullptr : "the slot loop was opened without it (ns2vc_sampler_open history2 = 1)",
                       h->stochastic ? nullptr : "the slot loop was opened without noise (ns2vc_sampler_open noise = 1)", h->x0c.mode,
                       ic.on && ic.n == ni ? ic.host.data() : nullptr))
    return 1;
  for (int k = 0; k < n; ++k) {      // what is the slot loop's own to say
    const int32_t* r = records + 4 * (size_t)k;
    const int b = slots[k];
    if (r[2] < h->next_step) return fail("slot %d: start %d lies in the past, the loop stands at step %d", b, r[2], h->next_step);
    if (r[2] > SOLVER_ITEM_NEVER - 1 - r[1])
      return fail("slot %d: loop steps %d + %d pass the end of the 32-bit step counter: drain the slots and call ns2vc_sampler_rebase", b, r[2], r[1]);
    for (int i = 0; i < r[1]; ++i)
      if (sl.coef[(size_t)(r[0] + i) * NS2VC_NCOEF + 1] == 0.f) return fail("slot %d: row %d of the table was never written (ns2vc_sampler_write_rows)", b, r[0] + i);
    if (h->guide.on && h->lens.masked && h->lens.applied[b] != h->lens.applied[b + ni]) return fail("guided slot loop: lengths[%d] and lengths[%d] differ", b, b + ni);
    if (h->shold.on && h->lens.masked && (int)h->shold.last.size() == ni && h->shold.last[(size_t)b] >= h->lens.applied[(size_t)b])      // (lengths set after the frames)
      return fail("known frame %d of slot %d lies at or past its length %d: set the known frames after the lengths", (int)h->shold.last[(size_t)b], b,
                  (int)h->lens.applied[(size_t)b]);
  }
  hipStream_t s = (hipStream_t)stream;
  const int* slots_dev = nullptr;
  const SolverItem* rec_dev = nullptr;
  if (stage_slot_list(h, n, slots, ni, rec, s, &slots_dev, &rec_dev)) return 1;
  HIPCHK(launch_sampler_admit(x_T_nct, h->cfg.latent_channels, h->T, n, slots_dev, ni, rec_dev, h->items.dev, h->xe, h->xe_op, h->prec, h->xbar, h->d1,
                              h->mprev, h->hist2.on ? h->hist2.dev : nullptr, h->CP, h->pair_off(), h->lens.masked ? h->lens.dev : nullptr,
                              h->guide.on ? ni : 0, s));
  for (int k = 0; k < n; ++k) {
    sl.rec[slots[k]] = rec[k];
    sl.busy[slots[k]] = 1;
    h->steps = std::max(h->steps, rec[k].start + rec[k].steps);      // S follows the admissions
  }
  return 0;
}

int ns2vc_sampler_take(ns2vc_unet* h, int n, const int32_t* slots, float* x_out_nct, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (!x_out_nct) return fail("null tensor");
  auto& sl = h->slots;
  const int ni = h->loop_items();
  if (!slots || n <= 0 || n > ni) return fail("a slot list needs 1 .. %d entries, got %d", ni, n);
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    if (b < 0 || b >= ni) return fail("slots[%d] = %d outside [0, %d)", k, b, ni);
    if (!sl.busy[b]) return fail("slot %d is idle: nothing to take", b);
    if (h->next_step < sl.rec[b].start + sl.rec[b].steps)
      return fail("slot %d has not finished: it runs until loop step %d, the loop stands at %d", b, sl.rec[b].start + sl.rec[b].steps, h->next_step);
  }
  hipStream_t s = (hipStream_t)stream;
  const int* slots_dev = nullptr;
  if (stage_slot_list(h, n, slots, ni, nullptr, s, &slots_dev, nullptr)) return 1;
  HIPCHK(launch_sampler_take(h->xe, h->CP, h->cfg.latent_channels, h->T, n, slots_dev, ni, x_out_nct, h->items.dev, s));
  if (h->shold.on && (int)h->shold.last.size() == ni) {      // a slot's known frames last for one request: the same list, the clear form of the second launch
    HIPCHK(launch_known_items(nullptr, nullptr, h->cfg.latent_channels, h->T, n, slots_dev, ni, h->shold.known.dev, h->shold.mask.dev, h->CP, s));
    for (int k = 0; k < n; ++k) h->shold.last[(size_t)slots[k]] = -1;
  }
  for (int k = 0; k < n; ++k) {
    sl.rec[slots[k]] = solver_item_idle();
    sl.busy[slots[k]] = 0;
  }
  return 0;
}

// Suspend and resume of a running request.  The state of a slot is P planes of T rows of CP fp32 columns (xe, xbar, d1, mprev, and
// mprev2 in a loop opened with history 2) and its position done = loop step - start; everything else the caller holds and sends again.
int ns2vc_sampler_state_shape(ns2vc_unet* h, int* planes, int* T, int* ld) {
  if (need_slot_loop(h)) return 1;
  if (!planes || !T || !ld) return fail("null argument");
  *planes = h->hist2.on ? 5 : 4;
  *T = h->T;
  *ld = h->CP;
  return 0;
}

int ns2vc_sampler_suspend(ns2vc_unet* h, int n, const int32_t* slots, float* state_out_dev, int32_t* done_out_host, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (!state_out_dev || !done_out_host) return fail("null argument");
  if ((uintptr_t)state_out_dev & 15) return fail("the state buffer must be 16-byte aligned");
  auto& sl = h->slots;
  const int ni = h->loop_items();
  if ((int)sl.rec.size() != ni) return fail("the slot loop was opened for %d items, the loop has %d: open it again", (int)sl.rec.size(), ni);
  if (!slots || n <= 0 || n > ni) return fail("a slot list needs 1 .. %d entries, got %d", ni, n);
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    if (b < 0 || b >= ni) return fail("slots[%d] = %d outside [0, %d)", k, b, ni);
    if (!sl.busy[b]) return fail("slot %d is idle: nothing to suspend", b);
    const SolverItem& r = sl.rec[b];
    if (h->next_step < r.start) return fail("slot %d has not started: it begins at loop step %d, the loop stands at %d (take nothing, admit it later instead)", b, r.start, h->next_step);
    if (h->next_step - r.start >= r.steps)
      return fail("slot %d has finished (loop step %d of %d + %d): take it (ns2vc_sampler_take)", b, h->next_step, r.start, r.steps);
  }
  hipStream_t s = (hipStream_t)stream;
  const int* slots_dev = nullptr;
  if (stage_slot_list(h, n, slots, ni, nullptr, s, &slots_dev, nullptr)) return 1;
  HIPCHK(launch_sampler_suspend(h->xe, h->xbar, h->d1, h->mprev, h->hist2.on ? h->hist2.dev : nullptr, h->T, h->CP, n, slots_dev, ni, state_out_dev,
                                h->items.dev, s));
  if (h->shold.on && (int)h->shold.last.size() == ni) {      // the request leaves with its known frames, as on a take: resume sends them again
    HIPCHK(launch_known_items(nullptr, nullptr, h->cfg.latent_channels, h->T, n, slots_dev, ni, h->shold.known.dev, h->shold.mask.dev, h->CP, s));
    for (int k = 0; k < n; ++k) h->shold.last[(size_t)slots[k]] = -1;
  }
  for (int k = 0; k < n; ++k) {
    done_out_host[k] = h->next_step - sl.rec[slots[k]].start;
    sl.rec[slots[k]] = solver_item_idle();
    sl.busy[slots[k]] = 0;
  }
  return 0;
}

// records: n x {row0, steps, done, flags}; the slot continues at row row0 + done with the next step (start = loop step - done)
int ns2vc_sampler_resume(ns2vc_unet* h, int n, const int32_t* slots, const float* state_in_dev, const int32_t* records, void* stream) {
  if (need_slot_loop(h)) return 1;
  if (!state_in_dev || !records) return fail("null argument");
  if ((uintptr_t)state_in_dev & 15) return fail("the state buffer must be 16-byte aligned");
  auto& sl = h->slots;
  const int ni = h->loop_items();
  if (h->items.n != ni || (int)sl.rec.size() != ni) return fail("the slot loop was opened for %d items, the loop has %d: open it again", h->items.n, ni);
  if (h->stochastic && !h->seeds.set) return fail("the slot loop takes stochastic items: set per-item seeds first (ns2vc_sampler_set_seeds)");
  if (!slots || n <= 0 || n > ni) return fail("a slot list needs 1 .. %d entries, got %d", ni, n);
  const SolverItem* in = reinterpret_cast<const SolverItem*>(records);      // (.start holds `done`)
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    if (b < 0 || b >= ni) return fail("slots[%d] = %d outside [0, %d)", k, b, ni);
    if (sl.busy[b]) return fail("slot %d is busy (admitted at loop step %d for %d steps, not taken yet): resume into an idle slot", b, sl.rec[b].start, sl.rec[b].steps);
    if (in[k].steps > 0 && (in[k].start < 0 || in[k].start >= in[k].steps))
      return fail("slot %d: done %d outside [0, %d): a request that has run all its rows is taken, not resumed", b, in[k].start, in[k].steps);
  }
  const auto& ic = h->x0c.items;
  if (solver_items_fit("slot", in, slots, n, kSlotRows, sl.coef.data(),
                       h->hist2.on ? nullptr : "the slot loop was opened without it (ns2vc_sampler_open history2 = 1)",
                       h->stochastic ? nullptr : "the slot loop was opened without noise (ns2vc_sampler_open noise = 1)", h->x0c.mode,
                       ic.on && ic.n == ni ? ic.host.data() : nullptr))
    return 1;
  std::vector<SolverItem> rec(in, in + n);
  for (int k = 0; k < n; ++k) {
    const int b = slots[k];
    SolverItem& r = rec[(size_t)k];
    r.start = h->next_step - in[k].start;      // in the past; below 0 after a rebase (done <= 1024: r - start cannot overflow)
    if (r.start > SOLVER_ITEM_NEVER - 1 - r.steps)
      return fail("slot %d: loop steps %d + %d pass the end of the 32-bit step counter: drain the slots and call ns2vc_sampler_rebase", b, r.start, r.steps);
    for (int i = 0; i < r.steps; ++i)
      if (sl.coef[(size_t)(r.row0 + i) * NS2VC_NCOEF + 1] == 0.f) return fail("slot %d: row %d of the table was never written (ns2vc_sampler_write_rows)", b, r.row0 + i);
    if (h->guide.on && h->lens.masked && h->lens.applied[b] != h->lens.applied[b + ni]) return fail("guided slot loop: lengths[%d] and lengths[%d] differ", b, b + ni);
    if (h->shold.on && h->lens.masked && (int)h->shold.last.size() == ni && h->shold.last[(size_t)b] >= h->lens.applied[(size_t)b])
      return fail("known frame %d of slot %d lies at or past its length %d: set the known frames after the lengths", (int)h->shold.last[(size_t)b], b,
                  (int)h->lens.applied[(size_t)b]);
  }
  hipStream_t s = (hipStream_t)stream;
  const int* slots_dev = nullptr;
  const SolverItem* rec_dev = nullptr;
  if (stage_slot_list(h, n, slots, ni, rec.data(), s, &slots_dev, &rec_dev)) return 1;
  HIPCHK(launch_sampler_resume(state_in_dev, h->T, h->CP, n, slots_dev, ni, rec_dev, h->items.dev, h->xe, h->xe_op, h->prec, h->xbar, h->d1, h->mprev,
                               h->hist2.on ? h->hist2.dev : nullptr, h->pair_off(), h->guide.on ? ni : 0, s));
  for (int k = 0; k < n; ++k) {
    sl.rec[slots[k]] = rec[(size_t)k];
    sl.busy[slots[k]] = 1;
    h->steps = std::max(h->steps, rec[(size_t)k].start + rec[(size_t)k].steps);
  }
  return 0;
}

int ns2vc_sampler_slot_step(ns2vc_unet* h, int* loop_step) {
  if (!h || !loop_step) return fail("null argument");
  *loop_step = h->in_slot_loop() ? h->next_step : -1;
  return 0;
}

}  // extern "C"
