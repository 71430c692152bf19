// cie_front.cpp -- a CIE1931 raster's way into the engine, timed on the host: one
// S x S image (default 4096: C3 size) of seeded random bytes in 2x2 blocks,
//   vectors  getBlocksAsVectorsFromImage + flatten + qvq_set_vectors, as CompressedImage::compress
//            did it for CIE1931 before qvq_set_images took the colour space (parts and total);
//   raster   qvq_set_images(..., QVQ_CS_CIE1931) (left out where the library refuses it);
//   compress CompressedImage::compress(image, LBG, CIE1931, 2, 2, eps, 8), its own compressionTime.
// Each leg once to warm up, then `reps` times; one JSON line with every timed call in ms.  Every
// timed call returns only when the engine is done with the rows.
//
//   g++ -O2 -std=c++17 -Iinclude tools/micro/cie_front.cpp -Lquant_amd/lib -lquant_amd -lqvq \
//       -Wl,-rpath,'$ORIGIN/../../quant_amd/lib' -o tools/micro/cie_front_new
// (and against another build's directory for an A/B).  usage: cie_front_new [S] [reps]
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "quant_amd/Compressor.hpp"
#include "qvq.h"

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static void print_list(const char *name, const std::vector<double> &v, bool last = false) {
    std::printf("\"%s\": [", name);
    for (size_t i = 0; i < v.size(); i++) std::printf("%s%.3f", i ? ", " : "", v[i]);
    std::printf("]%s", last ? "" : ", ");
}

int main(int argc, char **argv) {
    const int S = argc > 1 ? std::atoi(argv[1]) : 4096, reps = argc > 2 ? std::atoi(argv[2]) : 3;
    RGBImage image;
    image.xSize = image.ySize = S;
    image.img.resize((size_t)S * S);
    uint64_t z = 0x5EED;
    for (RGB &p : image.img)
        for (int c = 0; c < 3; c++) {
            z = z * 6364136223846793005ull + 1442695040888963407ull;
            p[c] = (char)(z >> 56);
        }
    qvq_ctx *ctx = nullptr;
    if (qvq_create(0, &ctx) != QVQ_OK) {
        std::fprintf(stderr, "qvq_create: %s\n", qvq_last_error(nullptr));
        return 1;
    }
    ColorSpacePtr cs = getColorSpace(ColorSpaces::CIE1931);
    std::vector<double> tile, flatten, upload, vectors, raster, compress;
    bool raster_ok = true;
    for (int r = 0; r <= reps; r++) {
        {
            const auto t0 = std::chrono::steady_clock::now();
            std::vector<Vector> blocks = getBlocksAsVectorsFromImage(image, 2, 2, cs);
            const double t_tile = ms_since(t0);
            const size_t N = blocks.size(), D = blocks[0].size();
            std::vector<double> flat(N * D);
            for (size_t i = 0; i < N; i++) std::copy(blocks[i].begin(), blocks[i].end(), flat.begin() + i * D);
            const double t_flat = ms_since(t0);
            if (qvq_set_vectors(ctx, flat.data(), N, (uint32_t)D) != QVQ_OK) {
                std::fprintf(stderr, "qvq_set_vectors: %s\n", qvq_last_error(ctx));
                return 1;
            }
            const double t_all = ms_since(t0);
            if (r) tile.push_back(t_tile), flatten.push_back(t_flat - t_tile), upload.push_back(t_all - t_flat),
                vectors.push_back(t_all);
        }
        if (raster_ok) {
            const auto t0 = std::chrono::steady_clock::now();
            const uint8_t *bytes = reinterpret_cast<const uint8_t *>(image.img.data());
            const qvq_status st = qvq_set_images(ctx, bytes, 1, (uint32_t)S, (uint32_t)S, 2, 2, QVQ_CS_CIE1931);
            if (st == QVQ_EUNSUPPORTED) {
                raster_ok = false;
            } else if (st != QVQ_OK) {
                std::fprintf(stderr, "qvq_set_images: %s\n", qvq_last_error(ctx));
                return 1;
            } else if (r) {
                raster.push_back(ms_since(t0));
            }
        }
    }
    qvq_destroy(ctx);
    for (int r = 0; r <= reps; r++) {
        const auto res = CompressedImage::compress(image, Quantizers::LBG, ColorSpaces::CIE1931, 2, 2, 1e-6, 8);
        if (r) compress.push_back(res.second.compressionTime.count() * 1e3);
    }
    std::printf("{\"side\": %d, \"raster_route\": %s, ", S, raster_ok ? "true" : "false");
    print_list("tile_ms", tile);
    print_list("flatten_ms", flatten);
    print_list("set_vectors_ms", upload);
    print_list("vectors_route_ms", vectors);
    print_list("raster_route_ms", raster);
    print_list("compress_ms", compress, true);
    std::printf("}\n");
    return 0;
}
