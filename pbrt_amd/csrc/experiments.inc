// experiments.inc -- measurement aids and measured-negative variants of the kernels, included by kernel_walk.hpp INSIDE the
// kernels' anonymous namespace.  Nothing here exists in the product build: every hook the kernels call expands to nothing unless the library
// is built with the switch named beside it (pbrt_amd/build.py PBRT_HIP_EXTRA_FLAGS="-D..."; tools/README.md):
//   PBRT_PHASE_PROBE     wave passes / active lanes per phase and a wave's s_memtime per section of render_kernel's loop
//   PBRT_RAY_LOG         every ray a frame traces, in launch order, to /tmp/raylog.bin (tools/raylog_probe.py)
//   PBRT_DEBUG_PIXEL_X/Y per-sample, per-bounce trace of one pixel (tools/debug_pixel.py diffs it against the oracle's)
//   PBRT_EXTRA_VALU=N    N extra independent v_fma_f32 per node step   } A-B sensitivity of the kernel to issue slots and
//   PBRT_EXTRA_LOADS     two re-issued 16-byte loads per node step     } to load instructions (DESIGN.md section 6)
//   PBRT_TRI_NT / PBRT_NODE_NT   r05: the walk's triangle / node fetches with the non-temporal hint (A-B of the L2's share between them)
//   PBRT_PREFETCH_POP    r03, measured negative (C3 -3.4 %, C2 -1.7 %, big -3.7 %: profiles/r03a_tree_prefetch_probes.txt): a
//                        parked lane requests one dword of the node below its stack top beside the triangle fetch

// ---- phase probe ----
#ifdef PBRT_PHASE_PROBE
__shared__ unsigned long long s_probe[24];
__device__ unsigned long long g_probe[24];
#define PROBE_ADD(i_, v_) do { const unsigned long long pv_ = (v_); if (threadIdx.x == 0) s_probe[i_] += pv_; } while (0)
// wave time (s_memtime cycles, stalls included) since the previous marker goes to section k_ (render_kernel's outer loop);
// the time of the last marker is kept in LDS and the first ACTIVE lane does the bookkeeping, so a marker inside a branch
// that lane 0 did not take still counts
#define PROBE_SEC(k_) do { const unsigned long long pt_ = __builtin_amdgcn_s_memtime(); \
    if ((int)(threadIdx.x & 63u) == __ffsll((long long)__ballot(true)) - 1) { s_probe[8 + (k_)] += pt_ - s_probe[23]; s_probe[23] = pt_; } } while (0)
// passes of a phase and the lanes active in them: counters i_ and i_ + 1
#define EXP_PROBE_LANES(i_, cond_) do { const unsigned long long pm_ = __ballot(cond_); if (pm_) { PROBE_ADD(i_, 1); PROBE_ADD((i_) + 1, __popcll(pm_)); } } while (0)
// flushes, and the passes they would take if the (lane, triangle) items were spread over all 64 lanes
#define EXP_PROBE_FLUSH(cnt_) do { uint32_t items_ = 0; for (uint32_t i_ = 0; i_ < 8; i_++) items_ += (uint32_t)__popcll(__ballot((cnt_) > i_)); \
    PROBE_ADD(6, 1); PROBE_ADD(7, (items_ + 63u) / 64u); } while (0)
#define EXP_PROBE_INIT(lane_) do { if ((lane_) < 24) s_probe[lane_] = (lane_) == 23 ? __builtin_amdgcn_s_memtime() : 0ull; } while (0)
#define EXP_PROBE_FINI(lane_) do { if ((lane_) < 23) atomicAdd(&g_probe[lane_], s_probe[lane_]); } while (0)
#define EXP_PROBE_INIT_BLOCK() do { if (threadIdx.x < 8) s_probe[threadIdx.x] = 0; __syncthreads(); } while (0)  // (thread 0 counts: wave 0 of the block is the sample)
#define EXP_PROBE_FINI_BLOCK() do { if (threadIdx.x < 8) atomicAdd(&g_probe[threadIdx.x], s_probe[threadIdx.x]); } while (0)
__global__ void probe_dump() {
  printf("PROBE step waves %llu lanes %llu | flush waves %llu lanes %llu | service waves %llu lanes %llu | flushes %llu dense passes %llu\n",
         g_probe[0], g_probe[1], g_probe[2], g_probe[3], g_probe[4], g_probe[5], g_probe[6], g_probe[7]);
  printf("PROBE wave cycles: traversal %llu | service: records+pixel %llu, shadow return / hit fetch / emission %llu, light sample %llu, bsdf + rr %llu, advance + film %llu, item fetch %llu, camera ray %llu, store + ray start %llu\n",
         g_probe[8], g_probe[9], g_probe[10], g_probe[11], g_probe[12], g_probe[13], g_probe[14], g_probe[15], g_probe[16]);
  for (int i = 0; i < 24; i++) g_probe[i] = 0;
}
#else
#define PROBE_SEC(k_) do { } while (0)
#define EXP_PROBE_LANES(i_, cond_) do { } while (0)
#define EXP_PROBE_FLUSH(cnt_) do { } while (0)
#define EXP_PROBE_INIT(lane_) do { } while (0)
#define EXP_PROBE_FINI(lane_) do { } while (0)
#define EXP_PROBE_INIT_BLOCK() do { } while (0)
#define EXP_PROBE_FINI_BLOCK() do { } while (0)
#endif

// ---- A-B sensitivity of the node step ----
#ifdef PBRT_EXTRA_LOADS
#define EXP_STEP_EXTRA_LOADS(quads_, off_, T_) do { uint4 X0_, X1_; const char *pp_ = (quads_) + (off_); \
    asm volatile("global_load_dwordx4 %0, %2, off\n\tglobal_load_dwordx4 %1, %2, off offset:32\n\ts_waitcnt vmcnt(0)" : "=&v"(X0_), "=&v"(X1_) : "v"(pp_) : "memory"); \
    if ((X0_.x ^ X1_.y) == 0x9e3779b9u && X0_.z == 0x12345u) (T_).tmax = 0.f; } while (0)
#else
#define EXP_STEP_EXTRA_LOADS(quads_, off_, T_) do { } while (0)
#endif
#ifdef PBRT_EXTRA_VALU
#define EXP_STEP_EXTRA_VALU(W0_, tfar_, T_) do { float x0_ = __uint_as_float((W0_).x), x1_ = __uint_as_float((W0_).y); \
    _Pragma("unroll") for (int k_ = 0; k_ < PBRT_EXTRA_VALU / 2; k_++) asm volatile("v_fma_f32 %0, %0, %2, %2\n\tv_fma_f32 %1, %1, %2, %2" : "+v"(x0_), "+v"(x1_) : "v"(tfar_)); \
    if (x0_ == 1.2345f && x1_ == 5.4321f) (T_).tmax = 0.f; } while (0)
#else
#define EXP_STEP_EXTRA_VALU(W0_, tfar_, T_) do { } while (0)
#endif

// ---- r05: cache policy of the walk's two fetches (PBRT_TRI_NT / PBRT_NODE_NT: the non-temporal hint on the triangle records / the nodes) ----
#if defined(PBRT_TRI_NT) || defined(PBRT_NODE_NT)
typedef float exp_f32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t exp_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 exp_nt_load(const float4 *p) { const exp_f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const exp_f32x4 *>(p)); return make_float4(v.x, v.y, v.z, v.w); }
__device__ __forceinline__ uint4 exp_nt_load(const uint4 *p) { const exp_u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const exp_u32x4 *>(p)); return make_uint4(v.x, v.y, v.z, v.w); }
#endif
#ifdef PBRT_TRI_NT
#define EXP_TRI_LOAD(p_) exp_nt_load(p_)
#else
#define EXP_TRI_LOAD(p_) (*(p_))
#endif
#ifdef PBRT_NODE_NT
#define EXP_NODE_LOAD(p_) exp_nt_load(p_)
#else
#define EXP_NODE_LOAD(p_) (*(p_))
#endif

// ---- r03: prefetch of the node a parked lane will pop (measured negative) ----
#ifdef PBRT_PREFETCH_POP
// (kept live until after the leaf pass so that the load's register is not reused under it; entries beyond the LDS part of an
// overflow stack are not followed)
#define EXP_LEAF_PREFETCH_BEGIN(parked_, quads_, T_) uint32_t pf_ = 0u; \
    if (parked_) { const uint32_t top_ = lds_load((T_).sp - kRowBytes); if (!(top_ & kLeafRef)) pf_ = *reinterpret_cast<const uint32_t *>((quads_) + top_); }
#define EXP_LEAF_PREFETCH_END() asm volatile("" ::"v"(pf_))
#else
#define EXP_LEAF_PREFETCH_BEGIN(parked_, quads_, T_) do { } while (0)
#define EXP_LEAF_PREFETCH_END() do { } while (0)
#endif

// ---- per-pixel trace (uses render_kernel's R, xr, yr) ----
#ifdef PBRT_DEBUG_PIXEL_X
#define EXP_DEBUG_PIXEL(...) do { if (R.sx0 + xr == PBRT_DEBUG_PIXEL_X && R.sy0 + yr == PBRT_DEBUG_PIXEL_Y) printf(__VA_ARGS__); } while (0)
#else
#define EXP_DEBUG_PIXEL(...) do { } while (0)
#endif

// ---- ray log ----
#ifdef PBRT_RAY_LOG
__device__ float4 *g_raylog = nullptr;
__device__ unsigned long long g_raylog_n = 0, g_raylog_cap = 0;
#define EXP_RAY_LOG(launch_, ro_, rd_, rtmax_, any_) do { if ((launch_) && g_raylog) { const unsigned long long k_ = atomicAdd(&g_raylog_n, 1ull); \
    if (k_ < g_raylog_cap) { g_raylog[2 * k_] = make_float4((ro_).x, (ro_).y, (ro_).z, (rtmax_)); \
                             g_raylog[2 * k_ + 1] = make_float4((rd_).x, (rd_).y, (rd_).z, (any_) ? 1.f : 0.f); } } } while (0)
#else
#define EXP_RAY_LOG(launch_, ro_, rd_, rtmax_, any_) do { } while (0)
#endif

// ---- host side: what a launch of an experiment build does around the kernel ----
#if defined(PBRT_RAY_LOG)
constexpr bool kExperimentLaunch = true;
static float4 *g_raylog_buf = nullptr;
static bool experiment_launch_begin(hipError_t *e) {  // true: give up with *e
  const unsigned long long cap = 160ull << 20, zero = 0;
  if (hipMalloc((void **)&g_raylog_buf, cap * 32) != hipSuccess) { *e = hipErrorOutOfMemory; return true; }
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_raylog), &g_raylog_buf, sizeof(g_raylog_buf));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_raylog_cap), &cap, sizeof(cap));
  (void)hipMemcpyToSymbol(HIP_SYMBOL(g_raylog_n), &zero, sizeof(zero));
  return false;
}
static void experiment_launch_end(hipStream_t stream) {
  (void)hipStreamSynchronize(stream);
  unsigned long long n = 0, cap = 0;
  (void)hipMemcpyFromSymbol(&n, HIP_SYMBOL(g_raylog_n), sizeof(n));
  (void)hipMemcpyFromSymbol(&cap, HIP_SYMBOL(g_raylog_cap), sizeof(cap));
  if (n > cap) n = cap;
  std::vector<float4> host(2 * n);
  (void)hipMemcpy(host.data(), g_raylog_buf, n * 32, hipMemcpyDeviceToHost);
  if (FILE *f = std::fopen("/tmp/raylog.bin", "wb")) { std::fwrite(host.data(), 32, n, f); std::fclose(f); }
  std::fprintf(stderr, "raylog: %llu rays -> /tmp/raylog.bin\n", n);
  (void)hipFree(g_raylog_buf);
  g_raylog_buf = nullptr;
}
#elif defined(PBRT_PHASE_PROBE)
constexpr bool kExperimentLaunch = true;
static bool experiment_launch_begin(hipError_t *) { return false; }
static void experiment_launch_end(hipStream_t stream) { probe_dump<<<1, 1, 0, stream>>>(); }
#else
constexpr bool kExperimentLaunch = false;
static bool experiment_launch_begin(hipError_t *) { return false; }
static void experiment_launch_end(hipStream_t) {}
#endif
