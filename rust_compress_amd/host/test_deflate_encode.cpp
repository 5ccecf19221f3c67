// test_deflate_encode.cpp -- the C++ twin's DEFLATE / zlib encoders (compress.hpp: flate::Encoder, zlib::Encoder) round-trip through
// its decoders.  Needs a GPU; run by tests/test_gpu_deflate_encode.py.
//   g++ -std=c++17 test_deflate_encode.cpp -L../csrc -lrcx -Wl,-rpath,../csrc -o test_deflate_encode && ./test_deflate_encode
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include "compress.hpp"

using namespace compress;
typedef std::vector<uint8_t> Bytes;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

int main()
{
    std::mt19937 rng(5);
    std::vector<Bytes> inputs = {Bytes(), Bytes{'a'}, Bytes(100000, 'z')};
    Bytes txt;
    const char* words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "lazy ", "dog ", "\n"};
    while (txt.size() < 200000) { const char* w = words[rng() % 9]; txt.insert(txt.end(), w, w + strlen(w)); if (rng() % 4 == 0) txt.push_back((uint8_t)('a' + rng() % 26)); }
    inputs.push_back(txt);
    for (const Bytes& in : inputs) {
        zlib::Encoder<VecWriter> ez{VecWriter()};
        for (size_t p = 0; p < in.size();) { const size_t k = std::min<size_t>(in.size() - p, 1 + rng() % 7000); ez.write(in.data() + p, k); p += k; }
        const Bytes z = ez.finish().v;
        CHECK(z.size() >= 6 && z[0] == 0x78 && ((z[0] << 8) | z[1]) % 31 == 0);
        zlib::Decoder<SliceReader> dz{SliceReader(z)};
        CHECK(dz.read_to_end() == in);
        flate::Encoder<VecWriter> ef{VecWriter()};
        ef.write_all(in.data(), in.size());
        const Bytes f = ef.finish().v;
        flate::Decoder<SliceReader> df{SliceReader(f)};
        CHECK(df.read_to_end() == in);
        CHECK(df.flags == 0);
    }
    printf("CPP_DEFLATE_ENCODE_OK\n");
    return 0;
}
