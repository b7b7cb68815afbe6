// The parser's look at APP1 (compeg_amd/csrc/front.cpp: exif_orientation) under g++ -fsanitize=address,undefined, built
// and run by tests/test_orient_emulation.py; a stand-alone program, never run on a GPU machine.
//
//   exif_driver FILE SEGMENT_OFFSET SEED
//
// FILE is a JPEG with an APP1 "Exif" segment whose marker stands at SEGMENT_OFFSET.  The program parses it, then again
// with every single byte of the segment's payload set to 0x00, to 0xFF and to a seeded random value, and with the file cut
// at every length inside the segment -- each time from a heap block of exactly the file's size, so that a read beyond it
// is the sanitizer's to report.  The orientation must always be 1..8; while the mutation lies inside the payload the return
// code and the message must be the unmutated file's.  Prints "ok N" (N parses) and returns 0, or says what differed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "front.h"

using namespace compeg;

struct Outcome {
    int code;
    std::string message;
    uint32_t orientation;
};

static Outcome parse(const std::vector<uint8_t> &file)
{
    // (exactly as long as the file: the vector's capacity may be larger)
    uint8_t *block = static_cast<uint8_t *>(malloc(file.size() ? file.size() : 1));
    if (!block)
        abort();
    memcpy(block, file.data(), file.size());
    ImageData *img = nullptr;
    const Status s = ImageData::parse(block, file.size(), false, &img);
    Outcome o{s.code, s.message, img ? img->orientation : 1u};
    delete img;
    free(block);
    return o;
}

int main(int argc, char **argv)
{
    if (argc != 4) {
        fprintf(stderr, "usage: exif_driver FILE SEGMENT_OFFSET SEED\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "rb");
    if (!f) {
        perror("open");
        return 2;
    }
    std::vector<uint8_t> file;
    for (int c; (c = fgetc(f)) != EOF;)
        file.push_back(uint8_t(c));
    fclose(f);
    const size_t at = strtoul(argv[2], nullptr, 0);
    uint64_t rng = strtoull(argv[3], nullptr, 0) * 2u + 1u;
    if (at + 4 > file.size() || file[at] != 0xff || file[at + 1] != 0xe1) {
        fprintf(stderr, "no APP1 at %zu\n", at);
        return 2;
    }
    const size_t payload = at + 4, end = at + 2 + (size_t(file[at + 2]) << 8 | file[at + 3]);
    if (end > file.size())
        return 2;
    const Outcome plain = parse(file);
    if (plain.orientation < 1u || plain.orientation > 8u) {
        fprintf(stderr, "unmutated: orientation %u\n", plain.orientation);
        return 1;
    }
    size_t parses = 1;
    for (size_t i = payload; i < end; i++) {
        rng = rng * 6364136223846793005ull + 1442695040888963407ull;
        const uint8_t values[3] = {0x00, 0xff, uint8_t(rng >> 56)};
        for (uint8_t v : values) {
            std::vector<uint8_t> m = file;
            m[i] = v;
            const Outcome o = parse(m);
            parses++;
            if (o.orientation < 1u || o.orientation > 8u || o.code != plain.code || o.message != plain.message) {
                fprintf(stderr, "byte %zu = 0x%02x: code %d (%s), orientation %u; unmutated: code %d (%s)\n", i, v, o.code, o.message.c_str(),
                        o.orientation, plain.code, plain.message.c_str());
                return 1;
            }
        }
    }
    // (a cut file is another file: whatever the parser says about it, it reads nothing beyond it and the tag stays 1..8)
    for (size_t n = at; n <= end; n++) {
        const Outcome o = parse(std::vector<uint8_t>(file.begin(), file.begin() + n));
        parses++;
        if (o.orientation < 1u || o.orientation > 8u) {
            fprintf(stderr, "cut at %zu: orientation %u\n", n, o.orientation);
            return 1;
        }
    }
    printf("ok %zu\n", parses);
    return 0;
}
