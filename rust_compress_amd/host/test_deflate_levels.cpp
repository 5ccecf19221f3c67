// test_deflate_levels.cpp -- the C++ twin's DEFLATE / zlib encoders at a compression level (compress.hpp: flate::Encoder,
// zlib::Encoder with a level) round-trip through its decoders, level 0 is the default encoder's bytes, a bad level throws.
// Needs a GPU; run by tests/test_gpu_deflate_levels.py.
//   g++ -std=c++17 test_deflate_levels.cpp -L../csrc -lrcx -Wl,-rpath,../csrc -o test_deflate_levels && ./test_deflate_levels
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
    std::mt19937 rng(9);
    std::vector<Bytes> inputs = {Bytes(), Bytes{'a'}, Bytes(100000, 'z')};
    Bytes txt;
    const char* words[] = {"the ", "quick ", "brown ", "fox ", "jumps ", "over ", "lazy ", "dog ", "\n"};
    while (txt.size() < 200000) { const char* w = words[rng() % 9]; txt.insert(txt.end(), w, w + strlen(w)); if (rng() % 4 == 0) txt.push_back((uint8_t)('a' + rng() % 26)); }
    inputs.push_back(txt);
    const uint8_t flevel[10] = {0x01, 0x01, 0x5e, 0x5e, 0x5e, 0x5e, 0x9c, 0xda, 0xda, 0xda};
    for (const Bytes& in : inputs) {
        size_t prev = 0;
        for (int level : {0, 1, 2, 6, 9}) {
            zlib::Encoder<VecWriter> ez{VecWriter(), level};
            ez.write_all(in.data(), in.size());
            const Bytes z = ez.finish().v;
            CHECK(z.size() >= 6 && z[0] == 0x78 && z[1] == flevel[level]);
            zlib::Decoder<SliceReader> dz{SliceReader(z)};
            CHECK(dz.read_to_end() == in);
            flate::Encoder<VecWriter> ef{VecWriter(), level};
            ef.write_all(in.data(), in.size());
            const Bytes f = ef.finish().v;
            flate::Decoder<SliceReader> df{SliceReader(f)};
            CHECK(df.read_to_end() == in);
            if (level == 1) {                                  // level 1 and the default: the same bytes
                flate::Encoder<VecWriter> e0{VecWriter()};
                e0.write_all(in.data(), in.size());
                CHECK(e0.finish().v == f);
            }
            if (level == 9) CHECK(f.size() <= prev);                   // (against level 1)
            if (level == 1) prev = f.size();
        }
    }
    for (int bad : {-1, 10}) {
        bool threw = false;
        try { flate::Encoder<VecWriter> e{VecWriter(), bad}; e.write_all(inputs[3].data(), 100); e.finish(); } catch (const std::exception&) { threw = true; }
        CHECK(threw);
    }
    printf("CPP_DEFLATE_LEVELS_OK\n");
    return 0;
}
