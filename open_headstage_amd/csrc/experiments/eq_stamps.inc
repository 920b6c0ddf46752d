// experiments build with -DOHS_EQ_STAMPS only (tools/eq_clock.py): shader-clock and 100 MHz real-time counters at the start /
// end of EVERY wave of EVERY k_eq_ring launch since the last reset, as a log of records {wave, samples of the launch, real
// time at start / end, shader clock at start / end}: a headline step is six launches of 512 waves, told apart on the host by
// their start times.  (The product has its own, one wave per launch: ohs_batch_profile_eq_clock.)
// Included by eq_kernels.hip inside namespace ohs.
constexpr unsigned kEqStampRecords = 16384;     // the log wraps: the host resets it in front of the step it reads
__device__ unsigned long long g_eq_stamps[6 * kEqStampRecords];
__device__ unsigned g_eq_stamp_count;
extern "C" int ohs_debug_eq_stamps_reset(void)
{
    const unsigned zero = 0;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_eq_stamp_count), &zero, sizeof(zero), 0, hipMemcpyHostToDevice);
}
// out: room for n_records x 6 values; *count = records written since the reset (more than kEqStampRecords: the log wrapped)
extern "C" int ohs_debug_eq_stamps(unsigned long long *out, size_t n_records, unsigned *count)
{
    if (n_records > kEqStampRecords) n_records = kEqStampRecords;
    hipError_t e = hipMemcpyFromSymbol(count, HIP_SYMBOL(g_eq_stamp_count), sizeof(unsigned), 0, hipMemcpyDeviceToHost);
    if (e == hipSuccess)
        e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_eq_stamps), n_records * 6 * sizeof(unsigned long long), 0, hipMemcpyDeviceToHost);
    return (int)e;
}
#define OHS_EQ_STAMP_BEGIN() const unsigned long long rt0 = __builtin_amdgcn_s_memrealtime(), ck0 = __builtin_amdgcn_s_memtime()
#define OHS_EQ_STAMP_END(wave_id)                                                    \
    do {                                                                             \
        const unsigned long long rt1 = __builtin_amdgcn_s_memrealtime(), ck1 = __builtin_amdgcn_s_memtime(); \
        if ((threadIdx.x & 63) == 0) {                                               \
            const unsigned slot = atomicAdd(&g_eq_stamp_count, 1u) % kEqStampRecords; \
            unsigned long long *rec = g_eq_stamps + 6ull * slot;                     \
            rec[0] = (unsigned long long)wave_id; rec[1] = (unsigned long long)n;    \
            rec[2] = rt0; rec[3] = rt1; rec[4] = ck0; rec[5] = ck1;                  \
        }                                                                            \
    } while (0)
