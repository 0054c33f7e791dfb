// thrust/random.h stand-in — TEST INFRASTRUCTURE (oracle/ref_pins only; never shipped).
//
// The two names the reference's src/interactions.{h,cu} use from Thrust, written from the
// published definitions (C++11 [rand.eng.lcong] minstd_rand and Thrust's documented
// uniform_real_distribution), so that interactions.cu compiles as host C++ without rocThrust
// (whose headers clash with the CUDA vector types on the include path of that build):
//   thrust::default_random_engine            minstd_rand: x <- 48271 * x mod (2^31 - 1),
//                                            seed(s): x = s mod m, 0 -> 1; min 1, max m - 1
//   thrust::uniform_real_distribution<float> (urng() - min) / (1 + (max - min)) * (b - a) + a,
//                                            evaluated in float, one engine draw per call
// Trusted because tests/test_bsdf_pin.py::test_standin_rng_reproduces_rocthrust compiles a
// program against this header and reproduces every entry of tests/golden/rng_pin.json, which
// oracle/ref_pins/rng_pin.cpp recorded from rocThrust itself.
#ifndef PT_THRUST_STANDIN_RANDOM_H
#define PT_THRUST_STANDIN_RANDOM_H

#include <cstdint>

namespace thrust {

class minstd_rand {
public:
    typedef std::uint32_t result_type;
    static const result_type multiplier = 48271u;
    static const result_type increment = 0u;
    static const result_type modulus = 2147483647u;
    static const result_type min = 1u;
    static const result_type max = modulus - 1u;
    static const result_type default_seed = 1u;

    explicit minstd_rand(result_type s = default_seed) { seed(s); }

    void seed(result_type s = default_seed) {
        m_x = s % modulus;
        if (m_x == 0u) m_x = default_seed;
    }

    result_type operator()() {
        m_x = static_cast<result_type>((static_cast<std::uint64_t>(m_x) * multiplier) % modulus);
        return m_x;
    }

    void discard(unsigned long long z) {
        for (; z > 0; --z) (*this)();
    }

private:
    result_type m_x;
};

typedef minstd_rand default_random_engine;

template <typename RealType = double>
class uniform_real_distribution {
public:
    typedef RealType result_type;

    explicit uniform_real_distribution(RealType a = RealType(0), RealType b = RealType(1)) : m_a(a), m_b(b) {}

    RealType a() const { return m_a; }
    RealType b() const { return m_b; }

    template <typename Engine>
    RealType operator()(Engine& urng) {
        RealType result = static_cast<RealType>(urng() - Engine::min);
        result /= (RealType(1) + static_cast<RealType>(Engine::max - Engine::min));
        return (result * (m_b - m_a)) + m_a;
    }

private:
    RealType m_a, m_b;
};

}  // namespace thrust

#endif  // PT_THRUST_STANDIN_RANDOM_H
