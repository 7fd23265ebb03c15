// sample_formats_iq.cpp -- float32_iq_code, the function the conversion kernel of FLOAT32_IQ input runs (csrc/sample_format.h,
// compiled for the host), on a file of float32 bit patterns: `sample_formats_iq <in> <out>` writes (uint16 code, uint16 what)
// pairs, which tests/test_iq_cpu.py holds against the numpy definition (adsbdec_amd/sample_formats.py flags_float32_iq).
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../adsbdec_amd/csrc/sample_format.h"

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out)
        return 2;
    std::vector<uint32_t> bits(1 << 16);
    std::vector<uint16_t> res(2 << 16);
    size_t n;
    while ((n = fread(bits.data(), 4, bits.size(), in)) > 0) {
        for (size_t i = 0; i < n; i++) {
            uint32_t what;
            res[2 * i] = (uint16_t)adsb::sample_code<adsb::kConvFloat32Iq>(bits[i], &what);
            res[2 * i + 1] = (uint16_t)what;
        }
        if (fwrite(res.data(), 2, 2 * n, out) != 2 * n)
            return 1;
    }
    return fclose(out) == 0 ? 0 : 1;
}
