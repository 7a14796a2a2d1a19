// Driver of tests/golden/make_sift_golden.py: runs the reference SIFT detector stage by stage on one raw
// 8-bit image and writes every intermediate result as named records.  Compiled by the generator against the
// reference's sfm/sift.cc and mve/image_tools.cc with -fno-access-control (the stages are private members);
// this file holds no reference code, only calls into it.
//
//   sift_golden_driver IMAGE.raw WIDTH HEIGHT CHANNELS MIN_OCTAVE OUT.bin [SAMPLES SIGMA]   stage dump
//   sift_golden_driver IMAGE.raw WIDTH HEIGHT CHANNELS MIN_OCTAVE --time N                  Sift::process, milliseconds per run
//
// SAMPLES, SIGMA: num_samples_per_octave and base_blur_sigma where a case sets them; the defaults otherwise.
//
// Record: u32 name length, name, u8 type ('f' float32, 'i' int32, 'b' uint8), u32 rows, u32 cols, data.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "mve/image.h"
#include "sfm/sift.h"

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

static void record_image(const std::string &name, mve::FloatImage::ConstPtr img)
{
    record(name, 'f', (uint32_t)img->height(), (uint32_t)img->width(), img->get_data_pointer());
}

static void record_keypoints(const std::string &name, const sfm::Sift::Keypoints &kps)
{
    std::vector<float> rows;
    for (const auto &k : kps) {
        rows.push_back((float)k.octave); rows.push_back(k.sample); rows.push_back(k.x); rows.push_back(k.y);
    }
    record(name, 'f', (uint32_t)kps.size(), 4, rows.data());
}

static bool by_scale(const sfm::Sift::Descriptor &a, const sfm::Sift::Descriptor &b) { return a.scale > b.scale; }

int main(int argc, char **argv)
{
    if (argc != 7 && argc != 8 && argc != 9) { fprintf(stderr, "usage: see the head of the source\n"); return 2; }
    const int w = atoi(argv[2]), h = atoi(argv[3]), c = atoi(argv[4]);
    mve::ByteImage::Ptr img = mve::ByteImage::create(w, h, c);
    FILE *in = fopen(argv[1], "rb");
    if (!in || fread(img->get_data_pointer(), 1, (size_t)w * h * c, in) != (size_t)w * h * c) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    fclose(in);
    sfm::Sift::Options opts;
    opts.min_octave = atoi(argv[5]);
    if (argc == 9) {
        opts.num_samples_per_octave = atoi(argv[7]);
        opts.base_blur_sigma = strtof(argv[8], nullptr);
    }

    if (!strcmp(argv[6], "--time")) {
        const int runs = atoi(argv[7]);
        std::vector<double> ms;
        size_t n = 0;
        for (int r = 0; r < runs; ++r) {
            sfm::Sift sift(opts);
            sift.set_image(img);
            const auto t0 = std::chrono::steady_clock::now();
            sift.process();
            ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
            n = sift.get_descriptors().size();
        }
        std::sort(ms.begin(), ms.end());
        printf("{\"descriptors\": %zu, \"process_ms_median\": %.3f, \"runs\": %d}\n", n, ms[ms.size() / 2], runs);
        return 0;
    }

    g_out = fopen(argv[6], "wb");
    if (!g_out) return 2;
    int32_t threw = 0;
    try {
        sfm::Sift sift(opts);
        sift.set_image(img);
        sift.create_octaves();
        for (size_t o = 0; o < sift.octaves.size(); ++o) {
            for (size_t i = 0; i < sift.octaves[o].img.size(); ++i)
                record_image("img/" + std::to_string(o) + "/" + std::to_string(i), sift.octaves[o].img[i]);
            for (size_t i = 0; i < sift.octaves[o].dog.size(); ++i)
                record_image("dog/" + std::to_string(o) + "/" + std::to_string(i), sift.octaves[o].dog[i]);
        }
        sift.extrema_detection();
        record_keypoints("candidates", sift.keypoints);
        sift.keypoint_localization();
        record_keypoints("keypoints", sift.keypoints);
        sift.descriptor_generation();
        sfm::Sift::Descriptors descr = sift.get_descriptors();
        for (int pass = 0; pass < 2; ++pass) {
            std::vector<float> meta, data;
            std::vector<uint8_t> colors;
            std::vector<float> norm;
            const float fw = (float)w, fh = (float)h, fnorm = std::max(fw, fh);
            for (const auto &d : descr) {
                meta.push_back(d.x); meta.push_back(d.y); meta.push_back(d.scale); meta.push_back(d.orientation);
                data.insert(data.end(), d.data.begin(), d.data.end());
                uint8_t px[3] = {0, 0, 0};
                img->linear_at(d.x, d.y, px);
                for (int k = 0; k < 3; ++k) colors.push_back(c == 3 ? px[k] : px[0]);
                norm.push_back((d.x + 0.5f - fw * 0.5f) / fnorm);
                norm.push_back((d.y + 0.5f - fh * 0.5f) / fnorm);
            }
            const std::string p = pass ? "sorted/" : "gen/";
            record(p + "meta", 'f', (uint32_t)descr.size(), 4, meta.data());
            record(p + "data", 'f', (uint32_t)descr.size(), 128, data.data());
            if (pass) {
                record(p + "colors", 'b', (uint32_t)descr.size(), 3, colors.data());
                record(p + "normalized", 'f', (uint32_t)descr.size(), 2, norm.data());
            }
            std::sort(descr.begin(), descr.end(), by_scale);
        }
    } catch (std::exception &e) {
        threw = 1;
    }
    record("threw", 'i', 1, 1, &threw);
    fclose(g_out);
    return 0;
}
