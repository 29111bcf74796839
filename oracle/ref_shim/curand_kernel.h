/* Stand-in for cuRAND's device API, for compiling the reference's header-only classes (R/*.h) as host C++
 * (oracle/ref_world.cpp): curandState, curand_init and curand_uniform of the XORWOW generator with the semantics DESIGN.md
 * section 2 "RNG" states -- salted seed, sequence = a jump of 2^67 steps, uniform = x * 2^-32 + 2^-33 in fp32.  tests/test_rng.py
 * pins the same step and jump to rocRAND's engine bit for bit; tests/test_reference_host.py pins this file to the oracle's.
 * The state is the six words {d, v0..v4} of rt_rng_state / Rng.state(), so a stream crosses the boundary as it is. */
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

struct curandState {
    uint32_t d;
    uint32_t v[5];
};

namespace ref_shim {

inline uint32_t Next(curandState* s)
{
    uint32_t t = s->v[0] ^ (s->v[0] >> 2);
    s->v[0] = s->v[1];
    s->v[1] = s->v[2];
    s->v[2] = s->v[3];
    s->v[3] = s->v[4];
    s->v[4] = (s->v[4] ^ (s->v[4] << 4)) ^ (t ^ (t << 1));
    s->d += 362437u;
    return s->v[4] + s->d;
}

/* One linear map of the 160 xorshift bits: row i is the image of bit i. */
struct Gf2 {
    uint32_t row[160][5];
    void Apply(const uint32_t in[5], uint32_t out[5]) const
    {
        uint32_t acc[5] = {0, 0, 0, 0, 0};
        for (int i = 0; i < 160; i++)
            if ((in[i >> 5] >> (i & 31)) & 1u)
                for (int k = 0; k < 5; k++) acc[k] ^= row[i][k];
        std::memcpy(out, acc, sizeof acc);
    }
    Gf2 Squared() const
    {
        Gf2 r;
        for (int i = 0; i < 160; i++) Apply(row[i], r.row[i]);
        return r;
    }
};

/* jumps[b] advances the xorshift part by 2^67 * 2^b steps (the Weyl counter d does not move with the sequence) */
inline const std::vector<Gf2>& SequenceJumps()
{
    static const std::vector<Gf2> jumps = [] {
        Gf2 m;
        for (int i = 0; i < 160; i++) {
            curandState s = {0, {0, 0, 0, 0, 0}};
            s.v[i >> 5] = 1u << (i & 31);
            Next(&s);
            std::memcpy(m.row[i], s.v, sizeof s.v);
        }
        for (int k = 0; k < 67; k++) m = m.Squared();
        std::vector<Gf2> out;
        for (int b = 0; b < 64; b++) {
            out.push_back(m);
            m = m.Squared();
        }
        return out;
    }();
    return jumps;
}

}  // namespace ref_shim

inline void curand_init(unsigned long long seed, unsigned long long sequence, unsigned long long offset, curandState* s)
{
    uint32_t s0 = (uint32_t)seed ^ 0xaad26b49u;
    uint32_t s1 = (uint32_t)(seed >> 32) ^ 0xf7dcefddu;
    uint32_t t0 = 1099087573u * s0;
    uint32_t t1 = 2591861531u * s1;
    s->d = 6615241u + t1 + t0;
    s->v[0] = 123456789u + t0;
    s->v[1] = 362436069u ^ t0;
    s->v[2] = 521288629u + t1;
    s->v[3] = 88675123u ^ t1;
    s->v[4] = 5783321u + t0;
    if (sequence) {
        const std::vector<ref_shim::Gf2>& jumps = ref_shim::SequenceJumps();
        for (int b = 0; b < 64; b++)
            if ((sequence >> b) & 1u) jumps[b].Apply(s->v, s->v);
    }
    for (unsigned long long k = 0; k < offset; k++) ref_shim::Next(s);   /* the reference only ever passes 0 */
}

inline float curand_uniform(curandState* s)
{
    return (float)ref_shim::Next(s) * 2.3283064e-10f + (2.3283064e-10f / 2.0f);
}

/* The CUDA toolkit's headers declare the float overloads of the math functions in the global namespace, so the reference's
 * `log(curand_uniform(randState))` (R/ConstantMedium.h:79) is the fp32 logarithm under its own toolchain; with <cmath> alone a
 * host compiler sees only ::log(double) there and would quietly take the fp64 one.  This overload stands in for the toolkit's:
 * the correctly rounded fp32 logarithm, the value DESIGN.md section 2 settles on (libdevice's own logf is not available here
 * and stays unpinned).  It is the only call of the headers with a float argument.  Build with -DREF_SHIM_DOUBLE_LOG to see
 * what the host overload would give. */
#ifndef REF_SHIM_DOUBLE_LOG
inline float log(float x) { return (float)::log((double)x); }
#endif
