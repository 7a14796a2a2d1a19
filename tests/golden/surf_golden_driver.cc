// Driver of tests/golden/make_surf_golden.py: runs the reference SURF detector stage by stage on one raw 8-bit
// image and writes every intermediate result as named records.  Compiled by the generator against the
// reference's sfm/surf.cc and mve/image_tools.cc with -fno-access-control (the stages are private members);
// this file holds no reference code, only calls into it.
//
//   surf_golden_driver IMAGE.raw WIDTH HEIGHT CHANNELS THRESHOLD UPRIGHT FORCED.f32 OUT.bin     stage dump
//   surf_golden_driver IMAGE.raw WIDTH HEIGHT CHANNELS THRESHOLD UPRIGHT --time N               Surf::process, ms per run
//
// FORCED.f32: float32 rows (x, y, scale, orientation, upright) on which descriptor_computation is called directly
// ("-" for none).  Record: u32 name length, name, u8 type ('f' float32, 'i' int32, 'b' uint8), u32 rows, u32 cols, data.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mve/image.h"
#include "mve/image_tools.h"
#include "sfm/surf.h"

static FILE *g_out;

static void record(const std::string &name, char type, uint32_t rows, uint32_t cols, const void *data)
{
    const uint32_t len = (uint32_t)name.size();
    fwrite(&len, 4, 1, g_out);
    fwrite(name.data(), 1, len, g_out);
    fwrite(&type, 1, 1, g_out);
    fwrite(&rows, 4, 1, g_out);
    fwrite(&cols, 4, 1, g_out);
    fwrite(data, type == 'b' ? 1 : 4, (size_t)rows * cols, g_out);
}

static void record_keypoints(const std::string &name, const sfm::Surf::Keypoints &kps)
{
    std::vector<float> rows;
    for (const auto &k : kps) {
        rows.push_back((float)k.octave); rows.push_back(k.sample); rows.push_back(k.x); rows.push_back(k.y);
    }
    record(name, 'f', (uint32_t)kps.size(), 4, rows.data());
}

static bool by_scale(const sfm::Surf::Descriptor &a, const sfm::Surf::Descriptor &b) { return a.scale > b.scale; }

int main(int argc, char **argv)
{
    if (argc != 9) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), c = atoi(argv[4]);
    mve::ByteImage::Ptr img = mve::ByteImage::create(w, h, c);
    FILE *in = fopen(argv[1], "rb");
    if (!in || fread(img->get_data_pointer(), 1, (size_t)w * h * c, in) != (size_t)w * h * c) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(in);
    sfm::Surf::Options opts;
    opts.contrast_threshold = (float)atof(argv[5]);
    opts.use_upright_descriptor = atoi(argv[6]) != 0;

    if (!strcmp(argv[7], "--time")) {
        const int runs = atoi(argv[8]);
        std::vector<double> ms;
        size_t n = 0;
        for (int r = 0; r < runs; ++r) {
            sfm::Surf surf(opts);
            const auto t0 = std::chrono::steady_clock::now();
            surf.set_image(img);
            surf.process();
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            n = surf.get_descriptors().size();
        }
        std::sort(ms.begin(), ms.end());
        printf("{\"descriptors\": %zu, \"set_image_and_process_ms_median\": %.3f, \"runs\": %d}\n", n, ms[ms.size() / 2], runs);
        return 0;
    }

    g_out = fopen(argv[8], "wb");
    if (!g_out) return 2;
    if (c == 3) {
        mve::ByteImage::Ptr grey = mve::image::desaturate<uint8_t>(img, mve::image::DESATURATE_LIGHTNESS);
        record("grey", 'b', (uint32_t)h, (uint32_t)w, grey->get_data_pointer());
    } else {
        record("grey", 'b', (uint32_t)h, (uint32_t)w, img->get_data_pointer());
    }
    sfm::Surf surf(opts);
    surf.set_image(img);
    surf.create_octaves();
    for (size_t o = 0; o < surf.octaves.size(); ++o)
        for (size_t k = 0; k < surf.octaves[o].imgs.size(); ++k) {
            mve::FloatImage::ConstPtr m = surf.octaves[o].imgs[k];
            record("map/" + std::to_string(o) + "/" + std::to_string(k), 'f', (uint32_t)m->height(), (uint32_t)m->width(),
                m->get_data_pointer());
        }
    surf.extrema_detection();
    record_keypoints("candidates", surf.keypoints);
    surf.keypoint_localization_and_filtering();
    record_keypoints("keypoints", surf.keypoints);
    surf.descriptor_assignment();
    sfm::Surf::Descriptors descr = surf.get_descriptors();
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<float> meta, data, trig, norm;
        std::vector<uint8_t> colors;
        const float fw = (float)w, fh = (float)h, fnorm = std::max(fw, fh);
        for (const auto &d : descr) {
            meta.push_back(d.x); meta.push_back(d.y); meta.push_back(d.scale); meta.push_back(d.orientation);
            data.insert(data.end(), d.data.begin(), d.data.end());
            trig.push_back(std::sin(d.orientation)); trig.push_back(std::cos(d.orientation));
            uint8_t px[3] = {0, 0, 0};
            img->linear_at(d.x, d.y, px);
            for (int k = 0; k < 3; ++k) colors.push_back(c == 3 ? px[k] : px[0]);
            norm.push_back((d.x + 0.5f - fw * 0.5f) / fnorm);
            norm.push_back((d.y + 0.5f - fh * 0.5f) / fnorm);
        }
        const std::string p = pass ? "sorted/" : "gen/";
        record(p + "meta", 'f', (uint32_t)descr.size(), 4, meta.data());
        record(p + "data", 'f', (uint32_t)descr.size(), 64, data.data());
        if (!pass) record(p + "trig", 'f', (uint32_t)descr.size(), 2, trig.data());
        if (pass) {
            record(p + "colors", 'b', (uint32_t)descr.size(), 3, colors.data());
            record(p + "normalized", 'f', (uint32_t)descr.size(), 2, norm.data());
        }
        std::sort(descr.begin(), descr.end(), by_scale);
    }

    // descriptor_computation on hand-placed inputs, and the sine and cosine this C library gives for them
    std::vector<float> forced;
    if (strcmp(argv[7], "-")) {
        FILE *f = fopen(argv[7], "rb");
        float row[5];
        while (f && fread(row, 4, 5, f) == 5) forced.insert(forced.end(), row, row + 5);
        if (f) fclose(f);
    }
    std::vector<float> fdata, ftrig;
    std::vector<int32_t> fok, fcoords;
    for (size_t i = 0; i < forced.size() / 5; ++i) {
        sfm::Surf::Descriptor d;
        d.x = forced[5 * i]; d.y = forced[5 * i + 1]; d.scale = forced[5 * i + 2]; d.orientation = forced[5 * i + 3];
        const bool upright = forced[5 * i + 4] != 0.0f;
        fok.push_back(surf.descriptor_computation(&d, upright) ? 1 : 0);
        fdata.insert(fdata.end(), d.data.begin(), d.data.end());
        const float sin_ori = upright ? 0.0f : std::sin(d.orientation), cos_ori = upright ? 1.0f : std::cos(d.orientation);
        ftrig.push_back(sin_ori);
        ftrig.push_back(cos_ori);
        // where the 400 samples fall: this file's own statement of the rounded, rotated grid (float, as the detector's)
        const int scale = (int)d.scale;
        for (int y = -10; y < 10; ++y)
            for (int x = -10; x < 10; ++x) {
                const float px = d.x + (cos_ori * (x + 0.5f) - sin_ori * (y + 0.5f)) * scale;
                const float py = d.y + (sin_ori * (x + 0.5f) + cos_ori * (y + 0.5f)) * scale;
                fcoords.push_back((int32_t)(px > 0.0f ? std::floor(px + 0.5f) : std::ceil(px - 0.5f)));
                fcoords.push_back((int32_t)(py > 0.0f ? std::floor(py + 0.5f) : std::ceil(py - 0.5f)));
            }
    }
    record("forced/in", 'f', (uint32_t)fok.size(), 5, forced.data());
    record("forced/ok", 'i', (uint32_t)fok.size(), 1, fok.data());
    record("forced/data", 'f', (uint32_t)fok.size(), 64, fdata.data());
    record("forced/trig", 'f', (uint32_t)fok.size(), 2, ftrig.data());
    record("forced/coords", 'i', (uint32_t)fok.size(), 800, fcoords.data());
    fclose(g_out);
    return 0;
}
