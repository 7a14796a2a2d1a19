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

#if defined(__HIPCC__)
#define OSFM_HOST_DEVICE __host__ __device__
#else
#define OSFM_HOST_DEVICE
#endif

// What the reference does to one track feature after the tracks are built, for one row of a view.  The mark's bits:
constexpr uint8_t kMarkIn = 1;          // the mask lets the row pass (a view without a mask: every row)
constexpr uint8_t kMarkOutside = 2;     // the reference's index lies outside the mask; such a row is masked out
constexpr int kClampReference = 0, kClampImage = 1;     // OSFM_CLAMP_REFERENCE, OSFM_CLAMP_IMAGE

// (int)fmax(fmin(v, hi), 0) of view.cpp:103-104 and common.cpp:302-303: the float position against an int bound,
// both promoted to double.  fmin and fmax return the other operand for a NaN, so the cast always sees a number.
OSFM_HOST_DEVICE inline int clamp_index(float v, int hi)
{
    const double d = (double)v, h = (double)hi;
    const double lo = d < h ? d : h;                       // fmin(d, h): a NaN position gives h
    const double r = lo > 0.0 ? lo : 0.0;                  // fmax(lo, 0)
    return (int)r;
}

// normalized[2] -> pixel_xy[2]: pixel_width * (pos + 0.5) on BOTH axes, in double, rounded to float, the expression
// of osfm_tracks_from_mve (matching_mve.cpp:461-463).
// mark: View::isPixelMaskedIn (view.cpp:100-112) on mask [mask_h][mask_w] (NULL: no mask, every row passes).  With
// kClampReference x is clamped by rows - 1 and y by cols - 1 as the reference does, and an index that then lies
// outside the mask -- where the reference reads past it -- masks the row out and sets kMarkOutside.
// rgb[3]: propagateColorsToTracks (common.cpp:289-315), the pixel of the import image under the truncated
// position; a grey image gives its value three times.
OSFM_HOST_DEVICE inline void view_mark_row(float nx, float ny, double pixel_width, const uint8_t *img, int width, int height,
    int channels, const uint8_t *mask, int mask_w, int mask_h, int clamp, int threshold, float *pixel_xy, uint8_t *mark,
    uint8_t *rgb)
{
    const float x = (float)(pixel_width * (nx + 0.5));
    const float y = (float)(pixel_width * (ny + 0.5));
    pixel_xy[0] = x; pixel_xy[1] = y;
    uint8_t m = kMarkIn;
    if (mask) {
        const int cx = clamp_index(x, (clamp == kClampImage ? mask_w : mask_h) - 1);
        const int cy = clamp_index(y, (clamp == kClampImage ? mask_h : mask_w) - 1);
        if (cx >= mask_w || cy >= mask_h) m = kMarkOutside;
        else m = (int)mask[(size_t)cy * mask_w + cx] > threshold ? kMarkIn : 0;
    }
    *mark = m;
    const int px = clamp_index(x, width - 1), py = clamp_index(y, height - 1);
    const uint8_t *p = img + ((size_t)py * width + px) * channels;
    for (int k = 0; k < 3; ++k) rgb[k] = channels == 3 ? p[k] : p[0];
}

// By scale descending, rows of equal scale in generation order: row i of the view is generation row order[i].
inline void feature_view_order(const std::vector<float> &scale, std::vector<int32_t> *order)
{
    order->resize(scale.size());
    std::iota(order->begin(), order->end(), 0);
    std::stable_sort(order->begin(), order->end(), [&scale](int32_t a, int32_t b) { return scale[(size_t)a] > scale[(size_t)b]; });
}

}  // namespace osfm
