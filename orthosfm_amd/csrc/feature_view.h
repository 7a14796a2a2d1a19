// FeatureSet's view of a detector's descriptors (feature_set.cc): the colour under each feature, its normalised
// position and the order by scale.  Shared by the SIFT and the SURF context, which keep descriptors in the order
// the detector generated them.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace osfm {

// Image<unsigned char>::linear_at with interpolate<unsigned char>'s + 0.5f truncation
inline void linear_at(const uint8_t *img, int w, int h, int ch, float x, float y, uint8_t *px)
{
    x = std::max(0.0f, std::min((float)(w - 1), x));
    y = std::max(0.0f, std::min((float)(h - 1), y));
    const int fx = (int)x, fy = (int)y;
    const int fx1 = std::min(fx + 1, w - 1), fy1 = std::min(fy + 1, h - 1);
    const float w1 = x - (float)fx, w0 = 1.0f - w1, w3 = y - (float)fy, w2 = 1.0f - w3;
    const size_t rs = (size_t)w * ch, r1 = fy * rs, r2 = fy1 * rs, c1 = (size_t)fx * ch, c2 = (size_t)fx1 * ch;
    for (int cc = 0; cc < ch; ++cc)
        px[cc] = (uint8_t)((float)img[r1 + c1 + cc] * (w0 * w2) + (float)img[r1 + c2 + cc] * (w1 * w2)
            + (float)img[r2 + c1 + cc] * (w0 * w3) + (float)img[r2 + c2 + cc] * (w1 * w3) + 0.5f);
}

// colors[3]: linear_at on the byte image (a grey image gives its value three times); normalized[2]:
// normalize_feature_positions with the principal point at (0.5, 0.5).
inline void feature_view_row(const uint8_t *pixels, int width, int height, int channels, float x, float y, uint8_t *colors,
    float *normalized)
{
    const float fw = (float)width, fh = (float)height, fnorm = std::max(fw, fh);
    uint8_t px[3] = {0, 0, 0};
    linear_at(pixels, width, height, channels, x, y, px);
    for (int k = 0; k < 3; ++k) colors[k] = channels == 3 ? px[k] : px[0];
    normalized[0] = (x + 0.5f - fw * 0.5f) / fnorm;
    normalized[1] = (y + 0.5f - fh * 0.5f) / fnorm;
}

// By scale descending, rows of equal scale in generation order: row i of the view is generation row order[i].
inline void feature_view_order(const std::vector<float> &scale, std::vector<int32_t> *order)
{
    order->resize(scale.size());
    std::iota(order->begin(), order->end(), 0);
    std::stable_sort(order->begin(), order->end(), [&scale](int32_t a, int32_t b) { return scale[(size_t)a] > scale[(size_t)b]; });
}

}  // namespace osfm
