// Driver of tests/golden/make_halve_golden.py: halves one raw 8-bit image with the reference's
// mve::image::rescale_half_size<uint8_t> and writes the result's bytes.  Compiled by the generator against the
// reference's headers; this file holds no reference code, only the call into it.
//
//   halve_golden_driver IMAGE.raw WIDTH HEIGHT CHANNELS OUT.raw
//
// Exit status 3: the reference refused the size (std::invalid_argument); OUT.raw is not written.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>

#include "mve/image.h"
#include "mve/image_tools.h"

int main(int argc, char **argv)
{
    if (argc != 6) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), c = atoi(argv[4]);
    mve::ByteImage::Ptr img = mve::ByteImage::create(w, h, c);
    FILE *in = fopen(argv[1], "rb");
    if (!in || fread(img->get_data_pointer(), 1, (size_t)w * h * c, in) != (size_t)w * h * c) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(in);
    mve::ByteImage::Ptr out;
    try {
        out = mve::image::rescale_half_size<uint8_t>(img);
    } catch (const std::invalid_argument &e) {
        fprintf(stderr, "refused: %s\n", e.what());
        return 3;
    }
    FILE *f = fopen(argv[5], "wb");
    if (!f) { fprintf(stderr, "cannot write %s\n", argv[5]); return 2; }
    fwrite(out->get_data_pointer(), 1, (size_t)out->width() * out->height() * out->channels(), f);
    fclose(f);
    return 0;
}
