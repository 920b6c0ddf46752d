#!/usr/bin/env python3
"""Prototype (not product): the quad form of the wave-ring EQ -- one band per quad of lanes, four VOP2+DPP instructions per
sample (tools/model_eq_quad_ring.py is the lane-level model and the specification) -- the twin of tools/proto_eq_wave_ring.py.

This script writes the steady-state loop as a stand-alone kernel, straight from the model's group_program(): K groups of 16
steps per iteration, the port's instructions in the slot that the DPP read-after-write hazard leaves free in every step
(alpha, delta, <slot>, beta, gamma), v_nop where a slot has nothing to carry.  Every encoding is 8 bytes and 8-byte aligned
except the group's s_waitcnt, which shares its slot with a 4-byte partner (s_nop, or the loop counter's s_add): 81 issue slots
per 16 samples = 5.06 per sample against the wave ring's 6.02 + port.  It builds tools/bin/proto_eq_quad_ring, and that program
(on the GPU box)
  * checks the outputs of three chains BIT FOR BIT against the host's DF2T cascade (parametric_eq.rs:116-122 order, every
    product and sum rounded separately: built with -ffp-contract=off), and
  * times 512 chains x 480 256 samples (one wave per workgroup) beside a lone wave's cycles per sample (s_memtime).
Head and tail of a launch and the state hand-over are the product's business: every chain has 96 zeros in front of its first
sample in both buffers (the ring starts from zero at group 5, one group before the first sample, exactly as the model starts
at group -1), and its length is a multiple of 16 K.

PROTO_VARIANT selects the loop, every one generated from the model's instruction list (tools/bin/proto_eq_quad_ring_<variant>):
    cur (default)   the product's loop of round 12: each of a group's three memory instructions alone in its slot
    nost / nold / nomem   attribution knock-outs: the stores / the load / all three replaced by v_nop -- the outputs are wrong
                    by construction, so these skip the bit check and only time (what does the port cost the loop?)
    C1 / C2 / C3    the cluster variants of the model's group_program(port=...): bit check and timing as for cur
    D1 / D2 / D1W / D2W   the merged variants (round 17): one store per group, one store and one load per two groups, and
                    each with the wait in front of the cluster; their offset registers are set up as the model's
                    ring_eq_as_launched sets them up
tools/ab_proto_eq_quad_port.sh runs them alternating in one call; profiles/r15_proto_eq_quad_port.txt and
profiles/r17_proto_eq_quad_port.txt are its tables.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import model_eq_quad_ring as model      # noqa: E402

K = int(os.environ.get("PROTO_K", str(model.K_DEFAULT)))
import gen_eq_quad_ring_asm as gen    # noqa: E402  (tools/ is on sys.path: this script's directory)

loop_asm = gen.loop_asm
VARIANT = os.environ.get("PROTO_VARIANT", "cur")
KNOCK_OUT = {"nost": ("buffer_store_dword",), "nold": ("buffer_load_dword",), "nomem": ("buffer_store_dword", "buffer_load_dword")}
assert VARIANT == "cur" or VARIANT in KNOCK_OUT or VARIANT in model.PORTS, VARIANT


def main():
    port = VARIANT if VARIANT in model.PORTS else None
    model.check_hazards(K, port=port)
    model.check_waits(K, port=port)
    body = gen.gen_loop(K, port=port)
    # (a knock-out keeps the slot: v_nop is the 8-byte encoding the loop has wherever a slot carries nothing)
    body = ["v_nop_e64" if l.startswith(KNOCK_OUT.get(VARIANT, ())) else l for l in body]
    slots = sum(1 for l in body if not l.startswith((".", "1:"))) - 4
    asm = "\n".join('        "' + l + '\\n"' for l in body)
    xdecl = "\n".join(f"    float x{k} = conv ? src[base + 16 * (G0 + {k}) + xs] : 0.0f;" for k in range(K))
    nx = K
    if port in model.PAIR_PORTS:        # v11: S, v12: X0 (row 3: group G0 + 1), v13 ..: the pairs (G0 + 2 j, G0 + 2 j + 1)
        nx = 1 + K // 2
        xdecl = "\n".join([xdecl.split("\n")[0], xdecl.split("\n")[1]] +
                          [f"    float x{1 + j} = pair ? src[base + 16 * (G0 + {2 * j}) + pxs] : 0.0f;" for j in range(1, K // 2)])
    xops = ", ".join(f'[x{k}] "+{{v{11 + k}}}"(x{k})' for k in range(nx))
    src = r'''
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
constexpr int NB = 10, K = %(K)d, G0 = 5, PAD = 16 * (G0 + 1);
constexpr bool CHECK = %(check)d;       // (a knock-out variant's outputs are wrong by construction)
constexpr int MERGED = %(merged)d;      // 1: one store per group (D1, D1W); 2: one store and one load per two groups (D2, D2W)
// raw buffer resource over `bytes` bytes (stride 0, DATA_FORMAT 32)
__device__ u32x4 rsrc(const void *p, unsigned bytes)
{
    const unsigned long long a = (unsigned long long)p;
    u32x4 v;
    v.x = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)a);
    v.y = (unsigned)__builtin_amdgcn_readfirstlane((int)((unsigned)(a >> 32) & 0xFFFFu));
    v.z = (unsigned)__builtin_amdgcn_readfirstlane((int)bytes);
    v.w = 0x00020000u;
    return v;
}
struct Coef { float b0[NB], b1[NB], b2[NB], a1[NB], a2[NB]; };

// one chain per wave (= per workgroup); chain c: src + c * stride, PAD zeros, then n = iters * 16 K - PAD samples
__global__ __launch_bounds__(64) void k(const float *src, float *dst, long long stride, int iters, Coef cf, unsigned long long *ticks)
{
    const int lane = threadIdx.x, q = lane >> 2, role = lane & 3;
    const bool band = q < NB, conv = q >= 12;
    const int j = band ? q : 0;
    // band quad: C1 = (1, 1, a2, a1), C2 = (b2, b1, b0, 1); pass-on and conveyor quads: C1 = (1, 1, 0, 0), C2 = (0, 0, 1, 1)
    const float C1 = role < 2 ? 1.0f : !band ? 0.0f : role == 2 ? cf.a2[j] : cf.a1[j];
    const float C2 = !band ? (role < 2 ? 0.0f : 1.0f) : role == 0 ? cf.b2[j] : role == 1 ? cf.b1[j] : role == 2 ? cf.b0[j] : 1.0f;
    const long long base = (long long)blockIdx.x * stride;
    const unsigned bytes = (unsigned)(iters * 16 * K * 4);
    const u32x4 rin = rsrc(src + base, bytes), rout = rsrc(dst + base, bytes);
    // model_eq_quad_ring.py: X_SAMPLE, STORE_SAMPLE
    const int xs = (role == 0 ? 71 : role == 1 ? 69 : role == 2 ? 62 : 60) - 4 * q;
    const int ss = (role == 0 ? 7 : 5) - 4 * q;
    unsigned voff_st = (q >= 12 && (role == 0 || role == 3)) ? (unsigned)(16 * (G0 - 1) + ss) * 4u : 0xFFFFF000u;
    unsigned voff_ld = conv ? (unsigned)(16 * G0 + xs) * 4u : 0xFFFFF000u;
    const bool st_lane = conv && (role == 0 || role == 3);
    unsigned inc_ld = conv ? 64u * K : 0u, inc_st = st_lane ? 64u * K : 0u;
    // the merged variants (model_eq_quad_ring.py: MSTORE_SAMPLE, PSTORE_SAMPLE, PX_SAMPLE; ring_eq_as_launched)
    const int row = lane >> 4, q3 = (lane | 32) >> 2;
    const bool pair = row == 1 || row == 3;
    const int ms = (role == 0 ? -1 : role == 1 ? -8 : role == 2 ? -10 : -3);
    const int pxs = (role == 0 ? 71 : role == 1 ? 69 : role == 2 ? 62 : 60) - 4 * q3 + (row == 3 ? 16 : 0);
    if (MERGED == 1) {
        voff_st = conv ? (unsigned)(16 * (G0 - 1) + 15 + ms - 4 * q) * 4u - 28u : 0xFFFFF000u;
        inc_st = inc_ld;
    } else if (MERGED == 2) {
        voff_st = pair ? (unsigned)(16 * G0 + 15 + ms - 4 * q3 - (row == 1 ? 16 : 0)) * 4u : 0xFFFFF000u;
        voff_ld = pair ? (unsigned)(16 * G0 + pxs) * 4u : 0xFFFFF000u;
        inc_ld = inc_st = pair ? 64u * K : 0u;
    }
    const unsigned long long mk = 0x9999999999999999ull;    // lanes a, d of every quad: the merge takes Zc there
%(xdecl)s
    float Z0 = 0.f, Z1 = 0.f, Zp = 0.f, Gr = 0.f, P = 0.f;
    unsigned cnt = 0u - (unsigned)iters;
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    asm volatile(
        "s_nop 4\n"
%(asm)s
        : [Z0] "+{v2}"(Z0), [Z1] "+{v3}"(Z1), [Zp] "+{v4}"(Zp), [Gr] "+{v5}"(Gr), [P] "+{v6}"(P), [vs] "+{v0}"(voff_st),
          [vl] "+{v1}"(voff_ld), %(xops)s, [cnt] "+s"(cnt)
        : [C1] "{v7}"(C1), [C2] "{v8}"(C2), [incl] "{v9}"(inc_ld), [incs] "{v10}"(inc_st), [rin] "s"(rin), [rout] "s"(rout), [mk] "s"(mk)
        : "memory", "scc", "vcc", "v20", "v21", "v22");
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    if (lane == 0 && ticks) ticks[blockIdx.x] = t1 - t0;
}

static void host_cascade(const Coef &c, const float *x, size_t n, std::vector<float> &y)
{
    float s1[NB] = {0}, s2[NB] = {0};
    y.resize(n);
    for (size_t i = 0; i < n; ++i) {
        float v = x[i];
        for (int b = 0; b < NB; ++b) {      // DF2T, parametric_eq.rs:116-122 / biquad 0.4.2: each operation rounds by itself
            const float out = s1[b] + c.b0[b] * v;
            s1[b] = (s2[b] + c.b1[b] * v) - c.a1[b] * out;
            s2[b] = c.b2[b] * v - c.a2[b] * out;
            v = out;
        }
        y[i] = v;
    }
}

int main()
{
    Coef c;
    for (int b = 0; b < NB; ++b) {          // peaking sections, RBJ, 48 kHz (any stable table does)
        const double f = 63.0 * std::pow(2.0, b * 0.85), q = 1.41, g = (b & 1) ? 2.5 : -3.0;
        const double A_ = std::pow(10.0, g / 40.0), w = 2.0 * M_PI * f / 48000.0, al = std::sin(w) / (2.0 * q), a0 = 1.0 + al / A_;
        c.b0[b] = (float)((1.0 + al * A_) / a0); c.b1[b] = (float)(-2.0 * std::cos(w) / a0); c.b2[b] = (float)((1.0 - al * A_) / a0);
        c.a1[b] = (float)(-2.0 * std::cos(w) / a0); c.a2[b] = (float)((1.0 - al / A_) / a0);
    }
    const int chains = 512, iters = (480256 + PAD + 64 + 16 * K - 1) / (16 * K);
    const long long total = (long long)iters * 16 * K, n = total - PAD - 64, stride = total + 64;   // the last 64 outputs are still in the ring
    std::vector<float> hx((size_t)chains * stride, 0.0f);
    unsigned long long sd = 0x0A5EAD00ull;
    for (int ch = 0; ch < chains; ++ch)
        for (long long i = 0; i < n; ++i) {
            sd = sd * 6364136223846793005ull + 1442695040888963407ull;
            hx[(size_t)ch * stride + PAD + i] = (float)((double)(sd >> 40) / 8388608.0 - 1.0);
        }
    float *dx, *dy; unsigned long long *dt;
    hipMalloc(&dx, hx.size() * 4); hipMalloc(&dy, hx.size() * 4); hipMalloc(&dt, chains * 8);
    hipMemcpy(dx, hx.data(), hx.size() * 4, hipMemcpyHostToDevice);
    hipMemset(dy, 0x7f, hx.size() * 4);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    float best = 1e30f;
    for (int rep = 0; rep < 6; ++rep) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(k, dim3(chains), dim3(64), 0, 0, dx, dy, stride, iters, c, dt);
        hipEventRecord(e1);
        if (hipEventSynchronize(e1) != hipSuccess) { printf("kernel failed: %%s\n", hipGetErrorString(hipGetLastError())); return 1; }
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (rep) best = ms < best ? ms : best;
        if (rep) printf("rep %%d: %%.4f ms\n", rep, ms);
    }
    std::vector<float> hy(hx.size());
    hipMemcpy(hy.data(), dy, hy.size() * 4, hipMemcpyDeviceToHost);
    int bad_total = 0;
    for (int ch : {0, 1, 511}) {
        if (!CHECK) { printf("chain %%3d: not checked (knock-out variant)\n", ch); continue; }
        std::vector<float> y;
        host_cascade(c, &hx[(size_t)ch * stride + PAD], (size_t)n, y);
        long long bad = 0, untouched = 0;
        for (long long i = 0; i < n; ++i) {
            const float got = hy[(size_t)ch * stride + PAD + i];
            unsigned gb; std::memcpy(&gb, &got, 4);
            untouched += gb == 0x7f7f7f7fu;
            bad += std::memcmp(&got, &y[i], 4) != 0 && !(y[i] == 0.0f && got == 0.0f);
        }
        long long stray = 0;                // nothing behind the chain's buffer, zeros in front of the first sample
        for (long long i = total; i < stride; ++i) { unsigned gb; std::memcpy(&gb, &hy[(size_t)ch * stride + i], 4); stray += gb != 0x7f7f7f7fu; }
        printf("chain %%3d: %%lld of %%lld samples differ from the host's DF2T cascade (%%lld never written, %%lld stray stores)\n", ch, bad, n, untouched, stray);
        bad_total += bad != 0 || stray != 0;
    }
    printf("variant %(variant)s: 512 chains x %%lld samples, one chain per wave: %%.3f ms = %%.2f ns per sample  (%%d issue slots per %%d samples = %%.3f per sample)\n",
           total, best, best * 1e6 / (double)total, %(slots)d, 16 * K, %(slots)d / (double)(16 * K));
    hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, dx, dy, stride, iters, c, dt);
    hipDeviceSynchronize();
    unsigned long long tk = 0; hipMemcpy(&tk, dt, 8, hipMemcpyDeviceToHost);
    printf("a lone wave: %%.3f s_memtime ticks per sample\n", (double)tk / (double)total);
    return bad_total ? 2 : 0;
}
''' % {"K": K, "asm": asm, "xdecl": xdecl, "xops": xops, "slots": slots, "check": int(VARIANT not in KNOCK_OUT), "variant": VARIANT,
       "merged": 1 if port in model.MERGED_PORTS else 2 if port in model.PAIR_PORTS else 0}
    tag = ("" if VARIANT == "cur" else "_" + VARIANT) + ("" if K == model.K_DEFAULT else f"_k{K}")
    path = f"/tmp/proto_eq_quad_ring{tag}.hip"
    open(path, "w").write(src)
    os.makedirs(os.path.join(HERE, "bin"), exist_ok=True)
    subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-w", "-ffp-contract=off", "--offload-arch=gfx950", "-o",
                    os.path.join(HERE, "bin", "proto_eq_quad_ring" + tag), path], check=True)
    print(f"built tools/bin/proto_eq_quad_ring{tag} (K = {K}, {VARIANT}); {slots} issue slots per {16 * K} samples")


if __name__ == "__main__":
    main()
