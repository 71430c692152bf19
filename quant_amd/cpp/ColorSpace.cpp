// Colour spaces; see include/quant_amd/ColorSpace.hpp.
#include "quant_amd/ColorSpace.hpp"

#include <cmath>
#include <cstdint>

#include "cie1931.hpp"

namespace {

// The reference converts the rounded double straight to char; on its x86 builds that keeps
// the low byte of the integer, which is what SCALED's (c - 128) * 255 relies on.
inline char low_byte(double rounded) { return (char)(uint8_t)((int64_t)rounded & 0xFF); }

class ScaledSpace : public ColorSpace {
public:
    RGBDouble RGBtoColorSpace(const RGB &c) override {
        RGBDouble r;
        for (int i = 0; i < 3; i++) r[i] = ((double)c[i] + 128.0) / 255;
        return r;
    }
    RGB colorSpaceToRGB(const RGBDouble &c) override {
        RGB r;
        for (int i = 0; i < 3; i++) r[i] = low_byte(std::round((c[i] - 128.0) * 255));
        return r;
    }
};

class Cie1931Space : public ColorSpace {
public:
    // the one statement of the map (quant_amd/csrc/cie1931.hpp), shared with the device kernel
    RGBDouble RGBtoColorSpace(const RGB &c) override {
        double v[3];
        qvq::cie1931_from_rgb((signed char)c[0], (signed char)c[1], (signed char)c[2], v);
        return {v[0], v[1], v[2]};
    }
    RGB colorSpaceToRGB(const RGBDouble &c) override {
        const double r = c[0] * 0.418 + c[1] * (-0.15866) + c[2] * (-0.082835);
        const double g = c[0] * (-0.091169) + c[1] * 0.25243 + c[2] * 0.015708;
        const double b = c[0] * 0.0009209 + c[1] * (-0.0025498) + c[2] * 0.17860;
        return {low_byte(std::round(r)), low_byte(std::round(g)), low_byte(std::round(b))};
    }
};

}  // namespace

RGBDouble ColorSpace::RGBtoColorSpace(const RGB &c) { return {(double)c[0], (double)c[1], (double)c[2]}; }

RGB ColorSpace::colorSpaceToRGB(const RGBDouble &c) {
    return {low_byte(std::round(c[0])), low_byte(std::round(c[1])), low_byte(std::round(c[2]))};
}

ColorSpacePtr getColorSpace(ColorSpaces cs) {
    switch (cs) {
    case ColorSpaces::NORMAL: return ColorSpacePtr(new ColorSpace());
    case ColorSpaces::SCALED: return ColorSpacePtr(new ScaledSpace());
    case ColorSpaces::CIE1931: return ColorSpacePtr(new Cie1931Space());
    }
    return nullptr;
}
