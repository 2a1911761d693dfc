// render_execute.cpp — running a frame of the render graph (struct soc_renderer, renderer.hpp): the second lane and its
// queue probe, the plan of a call (which passes run, on which lane, in which order, behind which waits: plan_frame, no HIP
// call) and the loop that issues it, the timing rings and the per-frame state setters.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "post_plan.hpp"
#include "renderer.hpp"

using namespace soc;

// The sky lane runs at high priority in this frame: chosen by the lane probe (or the knob), or one of the probe's
// high-priority windows. Evaluated inside the pass callbacks, after this call's frame_lane_probe.
bool soc::sky_lane_high(const soc_renderer* r) {
    return r->side_queue == 1 || (r->side_queue == -1 && r->lane_q[0] && r->side == r->lane_q[0]);
}
// SOC_RENDERER_BLOOM_IN_COMPOSITION in this frame: the bloom's last stage inside Composition where the sky lane is the
// critical path (high priority, as the lane probe's high windows too, so the probe times what would run), the fourth
// bloom pass then recording nothing. Both callbacks of a frame see the same lane (set before the passes are issued).
// Re-checked every frame: a frame whose globals resolution differs from the images takes Composition's generic
// path, which cannot compute the bloom, so the fourth pass must run then.
static bool bloom_in_comp_on_lane(const soc_renderer* r, bool high) {
    // SOC_RENDERER_BLOOM_IN_COMP_ANY_LANE=1: also beside the low-priority sky lane (measurement knob)
    return r->bloom_in_comp && r->bloom_in_comp_ok && (high || tuning_knob("SOC_RENDERER_BLOOM_IN_COMP_ANY_LANE", 0));
}
bool soc::bloom_in_comp_active(const soc_renderer* r) { return bloom_in_comp_on_lane(r, sky_lane_high(r)); }

// The fused histogram's 8 partial copies: allocated on the first PRE phase and cleared on the caller's stream
// BEFORE the second lane is forked, so the fork orders the clear ahead of the sky lane's sky_compose bins.
// (Round 2 cleared it with hipMemset on the null stream from inside the sky lane's pass: a non-blocking stream
// is not ordered after null-stream work, so a first frame's sky bins could land before the clear and be wiped,
// or land in stale memory: DESIGN.md §2.2.)
static int ensure_hist_scratch(soc_renderer* r, hipStream_t s) {
    if (r->hist_scratch) return SOC_OK;
    if (hipMalloc((void**)&r->hist_scratch, SOC_HISTOGRAM_SCRATCH_WORDS * sizeof(uint32_t)) != hipSuccess) {
        r->hist_scratch = nullptr;
        return set_error(SOC_E_HIP, "soc_renderer_execute: histogram scratch allocation failed");
    }
    if (hipMemsetAsync(r->hist_scratch, 0, SOC_HISTOGRAM_SCRATCH_WORDS * sizeof(uint32_t), s) != hipSuccess)
        return set_error(SOC_E_HIP, "soc_renderer_execute: histogram scratch clear failed");
    return SOC_OK;
}

static int upload_lights(soc_renderer* r, const soc_globals* g, hipStream_t s) {
    if (!r->img.d_globals) return set_error(SOC_E_INVALID_ARG, "soc_renderer_execute: lights need frame d_globals");
    if (!r->staging) {
        if (hipHostMalloc((void**)&r->staging, 4 * sizeof(soc_globals), 0) != hipSuccess)
            return set_error(SOC_E_HIP, "soc_renderer_execute: hipHostMalloc failed");
        for (auto& e : r->staging_ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                return set_error(SOC_E_HIP, "soc_renderer_execute: hipEventCreate failed");
    }
    const int slot = r->staging_slot;
    r->staging_slot = (slot + 1) & 3;
    (void)hipEventSynchronize(r->staging_ev[slot]);  // slot's previous copy has landed
    std::memcpy(&r->staging[slot], g, sizeof(soc_globals));
    hipError_t e = hipMemcpyAsync(r->img.d_globals, &r->staging[slot], sizeof(soc_globals), hipMemcpyHostToDevice, s);
    if (e != hipSuccess) return set_error(SOC_E_HIP, "soc_renderer_execute: globals upload: %s", hipGetErrorString(e));
    (void)hipEventRecord(r->staging_ev[slot], s);
    return SOC_OK;
}

// Flags of the renderer's cross-lane synchronisation events (a pass's `done`, the lane switch): they order CloudRendering /
// SkyCompose writes before the Composition / TAA reads on another hardware queue of a multi-XCD device, so they keep the
// default system-scope release (the L2 writeback an event record implies) (round 5 had made them fence-free
// for a gain within noise). SOC_RENDERER_EVENT_FENCE=1 drops the fence (hipEventDisableSystemFence), a measurement knob
// only. Timing events keep the default too: without the fence a start event's timestamp may be taken after the next kernel
// has begun (6.5 us into SSAO, tools/event_trace_check.py).
static unsigned device_event_flags() {
    return (unsigned)hipEventDisableTiming |
           (tuning_knob("SOC_RENDERER_EVENT_FENCE", 0) == 1 ? (unsigned)hipEventDisableSystemFence : 0u);
}

static int run_pass(soc_renderer::Pass& p, const soc_globals* g, hipStream_t s) {
    const int slot = p.next;
    if (p.timed) (void)hipEventRecord(p.ev0[slot], s);
    int rc = p.run(g, s);
    if (rc) return rc;
    if (p.timed) {
        (void)hipEventRecord(p.ev1[slot], s);
        p.last = slot;
        p.next = (slot + 1) % SOC_RENDERER_TIMING_RING;
        if (p.count < SOC_RENDERER_TIMING_RING) p.count++;
    }
    return SOC_OK;
}

// The second lane's stream(s) and events (all of them: a device change rebuilds the lane there).
void soc::destroy_side_lane(soc_renderer* r) {
    for (hipEvent_t* e : {&r->fork_ev, &r->join_ev, &r->switch_ev})
        if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    for (auto& e : r->probe_ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    if (r->lane_q[0] || r->lane_q[1]) {
        for (auto& q : r->lane_q)
            if (q) { (void)hipStreamDestroy(q); q = nullptr; }
    } else if (r->side) {
        (void)hipStreamDestroy(r->side);
    }
    r->side = nullptr;
    r->side_queue = -1;
    r->probe_frames = 0;
}

// HIP maps streams onto at most GPU_MAX_HW_QUEUES (4) hardware queues per priority, reusing the least-used queue once
// the pool is full. With RCCL's and torch's streams created first (a process group), a normal-priority second lane was
// given the caller's queue and the two lanes ran serialised (bench --exchange 0.79 vs 0.62 ms per frame, DESIGN.md §11
// r5.8). A stream of another priority comes from a pool of its own, so the lane keeps a queue of its own whatever the
// caller created. Which priority is faster depends on which lane is the frame's critical path (C3: the main lane, the
// sky lane low; C4 / C2: the sky lane, high is 3-10 % faster than low). The flags fix it (round 6: one queue per
// configuration, so a command runs the same kernels every time): low by default, SOC_RENDERER_SKY_LANE_HIGH high,
// SOC_RENDERER_SKY_LANE_PROBE the round-5 timed probe (frame_lane_probe: both timed over the first 273 frames). Tuning
// knob SOC_RENDERER_SIDE_QUEUE overrides (1 = high, 2 = low, 3 = probe, 0 = normal priority).
static int ensure_side_lane(soc_renderer* r) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return set_error(SOC_E_HIP, "soc_renderer_execute: hipGetDevice failed");
    if (r->side && r->side_device == dev) return SOC_OK;
    if (r->side) {   // the caller moved to another device: rebuild the lane (and its events) there
        destroy_side_lane(r);
        r->clouds_state.reset();   // the new lane is not ordered after the old one's clouds kernels
        for (auto& p : r->passes)
            if (p.done) { (void)hipEventDestroy(p.done); p.done = nullptr; p.done_recorded = false; }
    }
    // the lane's queue is fixed by the flags (deterministic: the same kernels every run): low priority by
    // default, high with SOC_RENDERER_SKY_LANE_HIGH, the timed probe only with SOC_RENDERER_SKY_LANE_PROBE
    const int sq_flags = (r->flags & SOC_RENDERER_SKY_LANE_HIGH) ? 1 : (r->flags & SOC_RENDERER_SKY_LANE_PROBE) ? 3 : 2;
    int sq = tuning_knob("SOC_RENDERER_SIDE_QUEUE", sq_flags);
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess || least == greatest) sq = 0;
    hipError_t se = hipSuccess;
    if (sq == 3) {
        se = hipStreamCreateWithPriority(&r->lane_q[0], hipStreamNonBlocking, greatest);
        if (se == hipSuccess) se = hipStreamCreateWithPriority(&r->lane_q[1], hipStreamNonBlocking, least);
        if (se == hipSuccess) se = hipEventCreateWithFlags(&r->switch_ev, device_event_flags());
        for (auto& e : r->probe_ev)
            if (se == hipSuccess) se = hipEventCreate(&e);
        r->side = r->lane_q[0];
        r->side_queue = -1;
        r->probe_frames = 0;
    } else if (const int cus = tuning_knob("SOC_RENDERER_SKY_CUS", 0); cus > 0 && cus < 32) {
        // measurement knob: the sky lane on a CU-masked queue of its own, `cus` of every 32 mask bits:
        // SOC_RENDERER_SKY_CU_LAYOUT 0 = bit i set when (i / 8) % 32 < cus (the driver hands mask bits to the XCDs
        // round-robin, so cus CUs of every XCD), 1 = when i % 32 < cus
        int dev_cus = 256;
        (void)hipDeviceGetAttribute(&dev_cus, hipDeviceAttributeMultiprocessorCount, dev);
        const int layout = tuning_knob("SOC_RENDERER_SKY_CU_LAYOUT", 0);
        std::vector<uint32_t> mask((size_t)(dev_cus + 31) / 32, 0u);
        for (int i = 0; i < dev_cus; ++i)
            if ((layout ? i % 32 : (i / 8) % 32) < cus) mask[(size_t)i / 32] |= 1u << (i % 32);
        se = hipExtStreamCreateWithCUMask(&r->side, (uint32_t)mask.size(), mask.data());
        r->side_queue = 0;
    } else if (sq == 1 || sq == 2) {
        se = hipStreamCreateWithPriority(&r->side, hipStreamNonBlocking, sq == 2 ? least : greatest);
        r->side_queue = sq;
    } else {
        se = hipStreamCreateWithFlags(&r->side, hipStreamNonBlocking);
        r->side_queue = 0;
    }
    if (se != hipSuccess ||
        hipEventCreateWithFlags(&r->fork_ev, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&r->join_ev, hipEventDisableTiming) != hipSuccess) {
        destroy_side_lane(r);
        return set_error(SOC_E_HIP, "soc_renderer_execute: second lane stream/event creation failed");
    }
    r->side_device = dev;
    return SOC_OK;
}

// Move the second lane to stream q: q waits for everything queued on the current lane stream, so the lane stays one
// in-order sequence (the passes' done events recorded on the old stream stay valid for waits).
static int switch_side_lane(soc_renderer* r, hipStream_t q) {
    if (q == r->side) return SOC_OK;
    if (hipEventRecord(r->switch_ev, r->side) != hipSuccess || hipStreamWaitEvent(q, r->switch_ev, 0) != hipSuccess)
        return set_error(SOC_E_HIP, "soc_renderer_execute: second lane switch failed");
    r->side = q;
    return SOC_OK;
}

// Auto mode's probe, at the start of each frame (a call with the PRE phase): after 16 frames left to the clocks, eight
// windows (32 frames at 4K, up to 128 for smaller frames: probe_window) run the sky lane at high, low, low, high, high,
// low, low, high priority; timing events on the caller's stream at each window's frame 8 and its end give its mean
// frame interval (the first 8 after a switch skipped). The ABBA order cancels a linear drift of the clocks over the probe (a plain high-then-low order read
// the warm-up as a slower high lane). High is kept only if its windows are faster by more than 2 % (C3 prefers low by
// ~1 %, C4 and C2 high by 3-10 % with the in-Composition bloom of high windows; at 1.5 % C3 took high in 2 of 6 runs,
// profiles/r05_ab_lane_probe.txt),
// once the last event has completed (queried, never waited on), for the renderer's life.
// Frames per probe window: 32 at 3840x2160 and above, more for smaller frames (their intervals are shorter, so a
// 32-frame window is within the timing noise), up to 128.
static int probe_window(const soc_renderer* r) {
    const long long px = (long long)r->img.color.width * r->img.color.height;
    if (px <= 0) return 32;
    return (int)std::min<long long>(128, std::max<long long>(32, 32LL * 8294400LL / px));
}
constexpr int kProbeStart = 16, kProbeWins = 8;
static int probe_end(const soc_renderer* r) { return kProbeStart + kProbeWins * probe_window(r); }

static int frame_lane_probe(soc_renderer* r, hipStream_t s) {
    if (r->side_queue != -1 || !r->lane_q[0]) return SOC_OK;
    const int kStart = kProbeStart, kWindow = probe_window(r), kSkip = 8, kEnd = probe_end(r);
    constexpr int kWins = kProbeWins;
    constexpr bool kHigh[kWins] = {true, false, false, true, true, false, false, true};
    const int f = r->probe_frames;
    if (f <= kEnd) {
        if (f >= kStart) {
            const int w = (f - kStart) / kWindow, o = (f - kStart) % kWindow;
            int slot = -1;
            if (o == kSkip && w < kWins) slot = 2 * w;
            else if (o == 0 && w > 0) slot = 2 * (w - 1) + 1;
            if (slot >= 0 && hipEventRecord(r->probe_ev[slot], s) != hipSuccess)
                return set_error(SOC_E_HIP, "soc_renderer_execute: lane probe event failed");
            if (o == 0 && w < kWins) {
                int rc = switch_side_lane(r, r->lane_q[kHigh[w] ? 0 : 1]);
                if (rc) return rc;
            }
        }
        r->probe_frames++;
        return SOC_OK;
    }
    if (hipEventQuery(r->probe_ev[2 * kWins - 1]) != hipSuccess) {   // not reached yet (or an error: the lane stays)
        (void)hipGetLastError();
        return SOC_OK;
    }
    float hi = 0.0f, lo = 0.0f;
    for (int w = 0; w < kWins; ++w) {
        float t = 0.0f;
        if (hipEventElapsedTime(&t, r->probe_ev[2 * w], r->probe_ev[2 * w + 1]) != hipSuccess) {
            (void)hipGetLastError();
            r->side_queue = 2;
            return switch_side_lane(r, r->lane_q[1]);
        }
        (kHigh[w] ? hi : lo) += t;
    }
    r->side_queue = (hi < 0.98f * lo) ? 1 : 2;
    return switch_side_lane(r, r->lane_q[r->side_queue - 1]);
}

// Lane of pass i with the second lane on or off: 0 = the caller's stream, 1 = the renderer's second lane.
static int static_lane(const soc_renderer* r, int i) {
    return (r->async && (r->passes[i].flags & SOC_PASS_ASYNC)) ? 1 : 0;
}

// An aborted frame (a pass or a caller pass returned an error after the fork): join the second lane so nothing of
// this call is left unordered against the caller's next work, and drop the frame's partial histograms (the resolve
// that would clear them did not run) so they are not counted into the next frame's exposure. The TAA history is
// not flipped: the next frame reads the last completed frame's history.
static int abort_frame(soc_renderer* r, hipStream_t s, bool forked, int rc) {
    if (forked && r->side && hipEventRecord(r->join_ev, r->side) == hipSuccess &&
        hipStreamWaitEvent(s, r->join_ev, 0) == hipSuccess)
        r->main_after_side = true;
    else if (forked)
        r->main_after_side = false;
    if (r->hist_scratch) (void)hipMemsetAsync(r->hist_scratch, 0, SOC_HISTOGRAM_SCRATCH_WORDS * sizeof(uint32_t), s);
    if (r->img.auto_exposure)
        (void)hipMemsetAsync(r->img.auto_exposure->histogram_buckets, 0, sizeof(r->img.auto_exposure->histogram_buckets), s);
    return rc;
}

// `out` into the caller's buffer, cut to cap - 1 characters; its whole length.
int64_t soc::copy_text(const std::string& out, char* buf, size_t cap) {
    if (buf && cap) {
        const size_t n = std::min(cap - 1, out.size());
        std::memcpy(buf, out.data(), n);
        buf[n] = 0;
    }
    return (int64_t)out.size();
}

// The host-known facts of a call, before any HIP call: whether the resolve folds the partial histograms itself (the call
// runs both phases) and, for a call with the PRE phase, whether the fused pair path applies at the globals' resolution.
static int frame_facts(soc_renderer* r, const soc_globals* g, int phase) {
    r->fold_in_resolve = (phase & SOC_PHASE_ALL) == SOC_PHASE_ALL && !(r->flags & SOC_RENDERER_UNFUSED_HISTOGRAM);
    if (!(phase & SOC_PHASE_PRE_EXPOSURE)) return SOC_OK;
    const bool pair_ok = soc::composition_pair_applicable(g, r->img.color, r->img.albedo, r->bloom_image(), r->img.normal,
                                                         r->img.depth, r->img.clouds);
    r->sky_split_active = r->sky_split && pair_ok;
    r->bloom_in_comp_ok = pair_ok;
    // the graph was derived with Composition independent of the clouds: it cannot fall back to reading them
    if (r->sky_split && !r->sky_split_active)
        return set_error(SOC_E_SHAPE, "soc_renderer_execute: globals resolution %dx%d differs from the frame images %dx%d",
                         g->resolution[0], g->resolution[1], r->img.color.width, r->img.color.height);
    return SOC_OK;
}

// SOC_BLOOM_SPARSE, decided once per frame (after the lane probe, like bloom_in_comp_active): the pair path at this
// frame's resolution (a generic-path Composition reads every pixel of the bloom output) and the knobs; the sparse
// last stage only where the in-kernel bloom does not replace it. `high`: the sky lane counts as high priority.
static void frame_bloom_decisions(soc_renderer* r, bool high) {
    const bool cells = r->bloom_in_comp && r->bloom_in_comp_ok && soc::bloom_sparse_applicable();
    r->bloom_sparse_frame = cells && r->bloom_sparse && !bloom_in_comp_on_lane(r, high);
    r->bloom_cells_frame = cells && (r->bloom_sparse_frame || bloom_in_comp_on_lane(r, high));
}

// The call runs pass i (its phase, and it has work).
static bool runs(const soc_renderer& r, int i, int phase) {
    const auto& p = r.passes[i];
    return (p.phase & phase) && !(p.skip && p.skip());
}

// The call runs a pass on the second lane (which then has to exist before the plan is issued).
static bool uses_side_lane(const soc_renderer& r, int phase) {
    for (int i = 0; i < (int)r.passes.size(); ++i)
        if (static_lane(&r, i) == 1 && runs(r, i, phase)) return true;
    return false;
}

// The plan of a call: every synchronisation step and pass of it, in issue order, into f.steps. Makes no HIP call and changes
// nothing but `f`. What it consults: the graph (phases, flags, derived edges and signals), r.async, r.flags,
// r.inputs_ordered, r.main_after_side, the passes' done_recorded, r.fold_in_resolve (through the passes' skip) and
// `ao_pos`, the value of SOC_RENDERER_SSAO_FIRST.
static void plan_frame(const soc_renderer& r, int phase, int ao_pos, FramePlan& f) {
    const int n = (int)r.passes.size();
    f.steps.clear();
    // lane of every pass run by this call (-1: not run)
    f.lane.assign(n, -1);
    f.lanes = false;
    for (int i = 0; i < n; ++i) {
        if (!runs(r, i, phase)) continue;
        f.lane[i] = static_lane(&r, i);
        f.lanes |= f.lane[i] == 1;
    }
    auto &lane = f.lane, &order = f.order, &pos = f.pos;
    auto &deps = f.deps, &ext = f.ext;
    for (auto* lists : {&deps, &ext}) {
        lists->resize(n);
        for (auto& l : *lists) l.clear();
    }
    // dependencies among the passes run by this call; a skipped pass (no work this call) hands its own
    // dependencies on to its dependents
    for (int i = 0; i < n; ++i) {
        const auto& p = r.passes[i];
        if (lane[i] < 0 && !(p.phase & phase)) continue;
        for (int j : p.deps) {
            if (lane[j] >= 0) deps[i].push_back(j);
            else if (r.passes[j].phase & phase) deps[i].insert(deps[i].end(), deps[j].begin(), deps[j].end());
        }
    }
    // Edges whose source is not run by this call, onto the other lane: the ring edges to the previous frame
    // (pass.carry) and this frame's edges to a pass of another phase's call (PRE -> POST of a multi-GPU frame).
    // Each waits on the source's latest `done` event; on the same lane stream order covers them.
    for (int i = 0; i < n; ++i) {
        if (lane[i] < 0) continue;
        const auto& p = r.passes[i];
        for (int j : p.carry)
            if (static_lane(&r, j) != lane[i]) ext[i].push_back(j);
        for (int j : p.deps)
            if (lane[j] < 0 && !(r.passes[j].phase & phase) && static_lane(&r, j) != lane[i]) ext[i].push_back(j);
    }
    // issue order (tuning knob SOC_RENDERER_SSAO_FIRST): the AO passes move within the main lane, ahead of passes they do
    // not depend on (same passes, same per-pass results). Default (-1): just before the last bloom pass, so SSAO's
    // 1024-lane workgroups start once the small bloom mips are done and overlap the sky lane's density / sun-visibility
    // kernels with the full-resolution upsample after them (C3 1370-1380 -> 1446-1451 fps, C2 +6 %, C4 +1 % against
    // AO first). 1: AO first; 0: registration order (AO after every bloom pass); k >= 2: after
    // k - 1 other passes. In a frame whose last bloom stage is sparse (SOC_BLOOM_SPARSE) the default is the registration
    // order: of the full-resolution upsample that -1 places behind the AO passes only the unproven strips are left, and with
    // the benchmark's all-zero emissive the chain in one piece measured C3 1965-1976 fps against 1937-1943 with -1 (the
    // parent's dense last stage: 1940-1945 with -1, 1897-1911 with 0); the box atrium's lamps 2450-2460 either way
    // (profiles/r09_ab_bloom_sparse.txt).
    order.resize(n);
    for (int i = 0; i < n; ++i) order[i] = i;
    if (ao_pos) {
        auto &ao = f.ao, &rest = f.rest;
        ao.clear();
        rest.clear();
        for (int i = 0; i < n; ++i) (r.passes[i].group == "Ambient Occlusion" ? ao : rest).push_back(i);
        bool free = !ao.empty();   // the AO passes may move only if none depends on an earlier non-AO pass
        for (int a : ao)
            for (int j : deps[a])
                if (r.passes[j].group != "Ambient Occlusion") free = false;
        if (free) {
            size_t at = 0;
            if (ao_pos >= 2) at = std::min(rest.size(), (size_t)(ao_pos - 1));
            if (ao_pos < 0)
                for (size_t k = 0; k < rest.size(); ++k)
                    if (r.passes[rest[k]].group == "Bloom") at = k;   // the last bloom pass
            order.assign(rest.begin(), rest.begin() + at);
            order.insert(order.end(), ao.begin(), ao.end());
            order.insert(order.end(), rest.begin() + at, rest.end());
        }
    }
    // The fork orders the second lane after everything the caller queued on `stream` before this call: the frame
    // inputs it wrote (e.g. the depth image), and the previous frame's main-lane passes that second-lane passes have
    // ring edges on (SkyCompose after TAA and the resolve). With SOC_RENDERER_STATIC_INPUTS the caller does not rewrite
    // the frame inputs between frames, so second-lane passes without such a ring edge (CloudRendering, which writes
    // only CLOUDS) run before the fork: the second lane starts the frame's clouds as soon as the previous frame's
    // second-lane work is done, overlapping the previous frame's composition and TAA.
    f.needs_fork.assign(n, 0);
    bool pre_fork = true;
    for (int oi = 0; oi < n; ++oi) {
        const int i = order[oi];
        if (lane[i] != 1) continue;
        bool carry_main = false;
        for (int j : r.passes[i].carry) carry_main |= static_lane(&r, j) == 0;
        if (!(r.flags & SOC_RENDERER_STATIC_INPUTS) || !r.inputs_ordered || carry_main) pre_fork = false;
        f.needs_fork[i] = !pre_fork;
    }
    // Each lane is one in-order stream, so a wait on the other lane's pass at position k (in this call's issue order on
    // that lane) also covers every earlier pass of it: waits already covered are not issued again (each costs the
    // waiting queue a barrier packet, ~10 us of idle measured between dependent kernels).
    auto step = [&f](FrameStep::Kind kind, int L, int pass = -1, int src = -1) {
        f.steps.push_back(FrameStep{kind, (uint8_t)L, (int16_t)pass, (int16_t)src});
    };
    pos.assign(n, -1);
    int next_pos[2] = {0, 0}, waited[2] = {-1, -1};
    bool forked_wait = false;
    if (f.lanes) step(FrameStep::Fork, 0);
    for (int oi = 0; oi < n; ++oi) {
        const int i = order[oi];
        if (lane[i] < 0) continue;
        const int L = lane[i];
        if (L == 1 && f.needs_fork[i] && !forked_wait) {
            step(FrameStep::ForkWait, 1, i);
            forked_wait = true;
        }
        for (int j : deps[i])
            if (lane[j] != L && pos[j] > waited[L]) {
                step(FrameStep::Wait, L, i, j);
                waited[L] = pos[j];
            }
        // ring edges and edges into another phase's call: sources of an earlier call. The second lane is ordered after
        // them by this call's fork; the caller's stream by the end of that earlier call (its join, or a main-lane wait
        // on the second lane's last pass), so a wait is issued only if that call ended without either. (`done` holds a
        // run once recorded: by an earlier call, or by this one further up the plan.)
        for (int j : ext[i])
            if (L == 0 && !r.main_after_side && (r.passes[j].done_recorded || (pos[j] >= 0 && r.passes[j].signal)))
                step(FrameStep::RingWait, L, i, j);
        step(FrameStep::Run, L, i);
        pos[i] = next_pos[L]++;
        if (r.passes[i].signal) step(FrameStep::Record, L, i);
    }
    // join (the caller's edge): everything of this call is ordered before whatever the caller queues next on `stream`.
    // Not issued when a main-lane pass already waited on the second lane's last pass.
    const bool side_joined = waited[0] >= next_pos[1] - 1;
    if (f.lanes && !side_joined) step(FrameStep::Join, 0);
}

// Carries the plan out, step by step. A step that fails after the fork ends the frame through abort_frame.
static int issue_plan(soc_renderer* r, const soc_globals* g, hipStream_t s) {
    // SOC_RENDERER_PROBE_SKIP_PASS=<pass name>: profiling only (wrong results), that pass launches nothing; bounds
    // what removing it (e.g. by fusing it into a neighbour) could gain in the frame
    static const char* probe_skip = getenv("SOC_RENDERER_PROBE_SKIP_PASS");
    for (const FrameStep& st : r->plan.steps) {
        hipStream_t ls = st.lane ? r->side : s;
        soc_renderer::Pass* p = st.pass >= 0 ? &r->passes[st.pass] : nullptr;
        int rc = SOC_OK;
        switch (st.kind) {
        case FrameStep::Fork:   // nothing of the frame is issued yet: no abort_frame
            if (hipEventRecord(r->fork_ev, s) != hipSuccess)
                return set_error(SOC_E_HIP, "soc_renderer_execute: second lane fork failed");
            break;
        case FrameStep::ForkWait:
            if (hipStreamWaitEvent(r->side, r->fork_ev, 0) != hipSuccess)
                rc = set_error(SOC_E_HIP, "soc_renderer_execute: second lane fork failed");
            break;
        case FrameStep::Wait:
        case FrameStep::RingWait:
            if (hipStreamWaitEvent(ls, r->passes[st.src].done, 0) != hipSuccess)
                rc = set_error(SOC_E_HIP, "soc_renderer_execute: %s: %s wait failed", p->name.c_str(),
                               st.kind == FrameStep::Wait ? "cross-lane" : "ring-edge");
            break;
        case FrameStep::Run:
            if (!(probe_skip && p->name == probe_skip)) rc = run_pass(*p, g, ls);
            break;
        case FrameStep::Record:
            if (!p->done && hipEventCreateWithFlags(&p->done, device_event_flags()) != hipSuccess)
                rc = set_error(SOC_E_HIP, "soc_renderer_execute: hipEventCreate failed");
            else if (hipEventRecord(p->done, ls) != hipSuccess)
                rc = set_error(SOC_E_HIP, "soc_renderer_execute: %s: event record failed", p->name.c_str());
            else
                p->done_recorded = true;
            break;
        case FrameStep::Join:
            if (hipEventRecord(r->join_ev, r->side) != hipSuccess || hipStreamWaitEvent(s, r->join_ev, 0) != hipSuccess)
                rc = set_error(SOC_E_HIP, "soc_renderer_execute: second lane join failed");
            break;
        }
        if (rc) return abort_frame(r, s, r->plan.lanes, rc);
    }
    return SOC_OK;
}

// The host-side state after a call that issued its whole plan.
static void frame_done(soc_renderer* r, int phase) {
    r->main_after_side = true;
    r->inputs_ordered = true;
    if (phase & SOC_PHASE_POST_EXPOSURE) r->hist = 1 - r->hist;   // ping-pong the TAA history
}

static int cascades_conflict(const soc_renderer* r, const char* who);

static int ssao_first(const soc_renderer* r) { return tuning_knob("SOC_RENDERER_SSAO_FIRST", r->bloom_sparse_frame ? 0 : -1); }

extern "C" int soc_renderer_execute(soc_renderer* r, const soc_globals* g, int32_t phase, soc_stream stream) {
    if (!r || !g) return set_error(SOC_E_INVALID_ARG, "soc_renderer_execute: null argument");
    hipStream_t s = hs(stream);
    const bool pre = phase & SOC_PHASE_PRE_EXPOSURE;
    int rc = frame_facts(r, g, phase);
    if (!rc && pre && r->has_cascades) {   // the atlas and the settings again: either may have changed since the record was set
        rc = soc::check_sun_cascades(&r->cascades, &r->img.shadow, "soc_renderer_execute");
        if (!rc) rc = cascades_conflict(r, "soc_renderer_execute");
    }
    // the fused histogram's partial copies, cleared on `s`
    if (!rc && pre && !(r->flags & SOC_RENDERER_UNFUSED_HISTOGRAM)) rc = ensure_hist_scratch(r, s);
    if (!rc && pre && (g->point_light_count || g->spot_light_count)) rc = upload_lights(r, g, s);
    if (!rc && uses_side_lane(*r, phase)) {
        rc = ensure_side_lane(r);
        if (!rc && pre) rc = frame_lane_probe(r, s);
    }
    if (rc) return rc;
    if (pre) frame_bloom_decisions(r, sky_lane_high(r));
    plan_frame(*r, phase, ssao_first(r), r->plan);
    rc = issue_plan(r, g, s);
    if (!rc) frame_done(r, phase);
    return rc;
}

// Test hook (not in the public header): the plan of soc_renderer_execute(r, g, phase) as text, one step per line,
// "kind<TAB>pass<TAB>lane<TAB>source pass", without a HIP call. `sky_lane_high`: the sky lane counts as high priority (in a
// real call the lane's queue decides). `advance`: afterwards the host-side state is that of a call that succeeded
// (inputs_ordered, main_after_side, done_recorded of the recording passes, the history slot), so that the next plan is the
// following call's. Returns the text's length (truncated to cap - 1 characters in `buf`), or an error code.
extern "C" int64_t soc_debug_plan_frame(soc_renderer* r, const soc_globals* g, int32_t phase, int32_t sky_lane_high,
                                        int32_t advance, char* buf, size_t cap) {
    if (!r || !g) return set_error(SOC_E_INVALID_ARG, "soc_debug_plan_frame: null argument");
    const int rc = frame_facts(r, g, phase);
    if (rc) return rc;
    if (phase & SOC_PHASE_PRE_EXPOSURE) frame_bloom_decisions(r, sky_lane_high != 0);
    plan_frame(*r, phase, ssao_first(r), r->plan);
    static const char* kKinds[] = {"fork", "fork_wait", "wait", "ring_wait", "run", "record", "join"};
    std::string out;
    for (const FrameStep& st : r->plan.steps) {
        out += kKinds[st.kind];
        out += '\t';
        if (st.pass >= 0) out += r->passes[st.pass].name;
        out += '\t';
        out += std::to_string((int)st.lane);
        out += '\t';
        if (st.src >= 0) out += r->passes[st.src].name;
        out += '\n';
        if (advance && st.kind == FrameStep::Record) r->passes[st.pass].done_recorded = true;
    }
    if (advance) frame_done(r, phase);
    return copy_text(out, buf, cap);
}

extern "C" float soc_renderer_pass_ms(soc_renderer* r, int32_t i) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size()) return -1.0f;
    auto& p = r->passes[i];
    if (!p.timed || p.last < 0) return -1.0f;
    float ms = -1.0f;
    if (hipEventElapsedTime(&ms, p.ev0[p.last], p.ev1[p.last]) != hipSuccess) return -1.0f;
    return ms;
}

// The "GPU Metric" record of the most recent frame (renderer.cpp:769-806): every timed pass's ms, summed
// into the reference's 12 groups (renderer.cpp:577-588; absent groups are 0), and their total.
extern "C" int64_t soc_renderer_metrics_json(soc_renderer* r, uint64_t frame, char* buf, size_t cap) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_metrics_json: null renderer");
    static const char* kGroups[12] = {"Depth Prepass", "Composition", "Tone Mapping", "Bloom", "Depth Of Field",
                                      "Shadows", "Rendering G-Buffer", "Screen Space Reflections", "Ambient Occlusion",
                                      "Auto Exposure", "Sky Rendering", "Temporal Anti-Aliasing"};
    double group_ms[12] = {0};
    double total = 0.0;
    std::string passes;
    for (int i = 0; i < (int)r->passes.size(); ++i) {
        const float ms = soc_renderer_pass_ms(r, i);
        if (ms < 0.0f) continue;
        total += ms;
        char item[160];
        std::snprintf(item, sizeof item, "%s\"%s\": %.6f", passes.empty() ? "" : ", ", r->passes[i].name.c_str(), ms);
        passes += item;
        for (int k = 0; k < 12; ++k)
            if (r->passes[i].group == kGroups[k]) group_ms[k] += ms;
    }
    std::string out = "{\"frame\": " + std::to_string(frame) + ", \"total_gpu_ms\": ";
    char num[64];
    std::snprintf(num, sizeof num, "%.6f", total);
    out += num;
    out += ", \"groups\": {";
    for (int k = 0; k < 12; ++k) {
        std::snprintf(num, sizeof num, "%s\"%s\": %.6f", k ? ", " : "", kGroups[k], group_ms[k]);
        out += num;
    }
    out += "}, \"passes\": {" + passes + "}}";
    return copy_text(out, buf, cap);
}

extern "C" int soc_renderer_set_pass_timing(soc_renderer* r, int32_t index, int32_t enable) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_pass_timing: null renderer");
    const int n = (int)r->passes.size();
    if (index < -1 || index >= n) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_pass_timing: bad index %d", index);
    for (int i = (index < 0 ? 0 : index); i < (index < 0 ? n : index + 1); ++i) {
        auto& p = r->passes[i];
        if (enable && p.ev0.empty()) {
            p.ev0.assign(SOC_RENDERER_TIMING_RING, nullptr);
            p.ev1.assign(SOC_RENDERER_TIMING_RING, nullptr);
            for (int k = 0; k < SOC_RENDERER_TIMING_RING; ++k)
                if (hipEventCreate(&p.ev0[k]) != hipSuccess || hipEventCreate(&p.ev1[k]) != hipSuccess)
                    return set_error(SOC_E_HIP, "soc_renderer_set_pass_timing: hipEventCreate failed");
        }
        p.timed = enable != 0;
    }
    return SOC_OK;
}

extern "C" int soc_renderer_reset_timing(soc_renderer* r) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_reset_timing: null renderer");
    for (auto& p : r->passes) { p.next = 0; p.count = 0; p.last = -1; }
    return SOC_OK;
}

extern "C" int soc_renderer_pass_stats(soc_renderer* r, int32_t i, float* total_ms, int32_t* frames) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size() || !total_ms || !frames)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_pass_stats: bad arguments");
    auto& p = r->passes[i];
    double sum = 0.0;
    for (int k = 0; k < p.count; ++k) {
        float ms = 0.0f;
        hipError_t e = hipEventElapsedTime(&ms, p.ev0[k], p.ev1[k]);
        if (e != hipSuccess) return set_error(SOC_E_HIP, "soc_renderer_pass_stats: %s", hipGetErrorString(e));
        sum += ms;
    }
    *total_ms = (float)sum;
    *frames = p.count;
    return SOC_OK;
}

extern "C" int32_t soc_renderer_side_queue(const soc_renderer* r) { return (r && r->side) ? r->side_queue : -1; }

extern "C" int32_t soc_renderer_side_queue_probe_frames(const soc_renderer* r) {
    if (!r || !r->async || tuning_knob("SOC_RENDERER_SIDE_QUEUE", 3) != 3) return 0;
    return probe_end(r) + 1;
}

extern "C" int32_t soc_renderer_pass_event_times(soc_renderer* r, int32_t i, void* base, float* start_ms, float* end_ms,
                                                 int32_t n) {
    if (!r || i < 0 || i >= (int32_t)r->passes.size() || !base || !start_ms || !end_ms || n < 0)
        return set_error(SOC_E_INVALID_ARG, "soc_renderer_pass_event_times: bad arguments");
    auto& p = r->passes[i];
    const int first = p.count < SOC_RENDERER_TIMING_RING ? 0 : p.next;   // the oldest recorded slot
    const int m = std::min(p.count, n);
    for (int k = 0; k < m; ++k) {
        const int slot = (first + (p.count - m) + k) % SOC_RENDERER_TIMING_RING;
        hipError_t e = hipEventElapsedTime(&start_ms[k], (hipEvent_t)base, p.ev0[slot]);
        if (e == hipSuccess) e = hipEventElapsedTime(&end_ms[k], (hipEvent_t)base, p.ev1[slot]);
        if (e != hipSuccess) return set_error(SOC_E_HIP, "soc_renderer_pass_event_times: %s", hipGetErrorString(e));
    }
    return m;
}

extern "C" int soc_renderer_set_async(soc_renderer* r, int32_t enable) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_async: null renderer");
    if (r->async != (enable != 0)) {
        // the second-lane passes move to another stream: the first call after it forks them behind the caller's stream
        // (SOC_RENDERER_STATIC_INPUTS would start CloudRendering ahead of the fork, beside the previous frame's clouds
        // kernels on the other stream, which share its workspace)
        r->inputs_ordered = false;
    }
    r->async = enable != 0;
    return SOC_OK;
}

extern "C" int soc_renderer_invalidate_cloud_tables(soc_renderer* r) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_invalidate_cloud_tables: null renderer");
    r->clouds_state.reset();   // the next CloudRendering rebuilds both tables and clears both counter blocks
    return SOC_OK;
}

extern "C" int soc_renderer_set_exposure_pixels(soc_renderer* r, uint64_t total_pixels, int32_t wide_accumulator) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_exposure_pixels: null renderer");
    r->total_pixels = total_pixels;
    r->wide = wide_accumulator;
    return SOC_OK;
}

extern "C" int soc_renderer_set_light_bounds(soc_renderer* r, const void* d_bounds, uint32_t flags) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_light_bounds: null renderer");
    if (flags & ~(uint32_t)SOC_LIGHTS_CULL) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_light_bounds: unknown flags %u", flags);
    r->light_bounds = d_bounds;
    r->light_flags = d_bounds ? flags : 0u;
    return SOC_OK;
}

// What cascades cannot be combined with (the cascaded kernels have no such forms), by name.
static int cascades_conflict(const soc_renderer* r, const char* who) {
    if (r->light_bounds) return set_error(SOC_E_UNSUPPORTED, "%s: sun cascades with bounded lights (soc_renderer_set_light_bounds) are not supported", who);
    if (r->flags & SOC_RENDERER_BLOOM_IN_COMPOSITION)   // the setting itself, whether or not it applies to this graph's extents
        return set_error(SOC_E_UNSUPPORTED, "%s: sun cascades with SOC_RENDERER_BLOOM_IN_COMPOSITION are not supported", who);
    return SOC_OK;
}

extern "C" int soc_renderer_set_sun_cascades(soc_renderer* r, const soc_sun_cascades* cascades) {
    static const char* P = "soc_renderer_set_sun_cascades";
    if (!r) return set_error(SOC_E_INVALID_ARG, "%s: null renderer", P);
    if (!cascades) {
        r->has_cascades = false;
        return SOC_OK;
    }
    if (!r->img.shadow.data) return set_error(SOC_E_INVALID_ARG, "%s: sun cascades need images.shadow (the atlas)", P);
    int rc = soc::check_sun_cascades(cascades, &r->img.shadow, P);
    if (!rc) rc = cascades_conflict(r, P);
    if (rc) return rc;
    r->cascades = *cascades;
    r->has_cascades = true;
    return SOC_OK;
}

extern "C" int32_t soc_renderer_current_history(const soc_renderer* r) { return r ? r->hist : -1; }

// Resume from a checkpoint (SURVEY.md §5 "Checkpoint / resume"): the slot whose history_color / history_velocity hold
// the previous frame's TAA result and velocity. The images and the AutoExposure block are caller-owned and restored by
// the caller; this is the renderer's one piece of temporal state.
extern "C" int soc_renderer_set_current_history(soc_renderer* r, int32_t index) {
    if (!r) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_current_history: null renderer");
    if (index != 0 && index != 1) return set_error(SOC_E_INVALID_ARG, "soc_renderer_set_current_history: index %d", index);
    r->hist = index;
    return SOC_OK;
}
