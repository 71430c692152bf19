// quant -- command-line front end of the MI355X codec, with the reference's flags and defaults
// (src/main.cpp:42-113, no Boost):
//
//   quant FILE -o OUT [-n bits=8] [-e eps=1e-6] [-w width=2] [-h height=2] [-r raport=0]
//                     [-q quantizer=0 (LBG; 1 median cut, 2 median cut + Lloyd)] [-c colorspace=1 (SCALED)]
//                     [--device N]
//                     [--refine N=0] [--fresh] [--reseed] [--lloyd N=0]
//
// FILE.ppm -> OUT.quant compresses, FILE.quant -> OUT.ppm decompresses, FILE.ppm -> OUT.ppm
// compresses and writes the decoded image (src/main.cpp:73-111); anything else prints "File
// type not supported" and exits 1.  Options take a value as "-n 8", "-n8", "--saveto OUT" or
// "--saveto=OUT" (program_options' short and long forms); -r takes a value ("-r 1"), -h is the
// block height and --help the help text, as in the reference.  The quantization itself runs
// on the GPU through libquant_amd.so / libqvq.so.  --refine N runs up to N Lloyd iterations at the
// final codebook size after the split levels (stopped by eps) and --fresh writes the indices of
// the codebook in the file (getRefinedLBGQuantizer); with neither the output is the reference's.
// --lloyd N runs up to N Lloyd iterations after every split (stopped by eps), the textbook schedule
// (getLloydLBGQuantizer, qvq_lbg_lloyd); --refine then continues from its result.
// --reseed (with --refine N > 0 or --lloyd N > 0) lets the iterations reseed their empty cells
// (QVQ_REFINE_RESEED, QVQ_LLOYD_RESEED).
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <map>
#include <stdexcept>
#include <string>

#include "quant_amd/Compressor.hpp"

namespace {

enum class FileType { NOT_SUPPORTED, PPM, QUANT };

// src/main.cpp:20-40: the extension after the last '.', unless a '/' comes first
FileType file_type(const std::string &path) {
    for (size_t i = path.size(); i-- > 0;) {
        if (path[i] == '/') return FileType::NOT_SUPPORTED;
        if (path[i] == '.') {
            const std::string ext = path.substr(i);
            if (ext == ".quant") return FileType::QUANT;
            if (ext == ".ppm") return FileType::PPM;
            return FileType::NOT_SUPPORTED;
        }
    }
    return FileType::NOT_SUPPORTED;
}

struct Params {   // include/ProgramParameters.hpp:5-19, defaults of src/main.cpp:49-57
    int n = 8, width = 2, height = 2, quantizer = (int)Quantizers::LBG, colorspace = (int)ColorSpaces::SCALED;
    float eps = 0.000001f;
    bool raport = false;
    int refine = 0;       // --refine: Lloyd iterations at the final K (0: none)
    bool fresh = false;   // --fresh: indices of the written codebook
    bool reseed = false;  // --reseed: the iterations reseed their empty cells
    int lloyd = 0;        // --lloyd: Lloyd iterations at every level (0: qvq_lbg's one assignment per level)
    bool kmeanspp = false;   // --init kmeans++: the codebook starts from k-means++ seeds (default split: LBG's schedule)
    bool kmeanspar = false;  // --init kmeans-par: ... from k-means|| seeds
    uint64_t seed = 0;       // --seed: of the k-means++ / k-means|| draws
    int trials = -1;         // --trials: greedy k-means++ with that many candidate rows a round (0: the default count)
    std::string file, saveto;
};

const char *kHelp =
    "Options:\n"
    "  --help                 Print help messages\n"
    "  -n arg (=8)            bits per codevector\n"
    "  -e arg (=9.99999997e-07) eps parameter for quantization algorithm\n"
    "  -w arg (=2)            Width of block\n"
    "  -h arg (=2)            Height of block\n"
    "  --file arg             File to compress/decompress\n"
    "  -o [ --saveto ] arg    Save to\n"
    "  -r arg (=0)            Print raport to std::out\n"
    "  -q [ --quantizer ] arg (=0) Pick quantizer: 0 LBG, 1 median cut, 2 median cut refined by\n"
    "                         up to 100 Lloyd iterations (stopped by -e); NORMAL and SCALED only\n"
    "  -c [ --colorspace ] arg (=1) Pick ColorSpace\n"
    "  --device arg (=0)      HIP device of the engine (MI355X build)\n"
    "  --refine arg (=0)      Lloyd iterations at the final codebook size (LBG, stopped by -e)\n"
    "  --fresh                Indices re-assigned to the written codebook\n"
    "  --reseed               Empty cells reseeded from the worst cells (with --refine or --lloyd)\n"
    "  --lloyd arg (=0)       Lloyd iterations after every split (LBG, stopped by -e)\n"
    "  --init arg (=split)    Starting codebook: split (LBG's schedule), kmeans++ (2^n training\n"
    "                         rows by D^2-sampling) or kmeans-par (the same from a few sampling\n"
    "                         passes, n <= 16), then --refine iterations; -q 0, not with --lloyd\n"
    "  --seed arg (=0)        Seed of the kmeans++ / kmeans-par draws\n"
    "  --trials arg           Greedy kmeans++: candidate rows drawn per round, the best is kept\n"
    "                         (0 .. 16, 0 = 2 + 7 floor(log2 K) / 10; with --init kmeans++)\n";

bool parse_bool(const std::string &v) {   // program_options' bool values
    if (v == "1" || v == "true" || v == "yes" || v == "on") return true;
    if (v == "0" || v == "false" || v == "no" || v == "off") return false;
    throw std::invalid_argument("the argument ('" + v + "') for option '-r' is invalid");
}

int parse_int(const std::string &v, const std::string &opt) {
    size_t pos = 0;
    const int x = std::stoi(v, &pos);
    if (pos != v.size()) throw std::invalid_argument("the argument ('" + v + "') for option '" + opt + "' is invalid");
    return x;
}

// Returns true when --help was given.
bool parse(int argc, char **argv, Params &p) {
    // option name -> canonical key; every option but --help takes a value
    const std::map<std::string, std::string> names = {
        {"-n", "n"}, {"-e", "e"}, {"-w", "w"}, {"-h", "h"}, {"-o", "o"}, {"--saveto", "o"}, {"-r", "r"},
        {"-q", "q"}, {"--quantizer", "q"}, {"-c", "c"}, {"--colorspace", "c"}, {"--c", "c"}, {"--file", "file"},
        {"--device", "device"}, {"--refine", "refine"}, {"--lloyd", "lloyd"},
        {"--init", "init"}, {"--seed", "seed"}, {"--trials", "trials"}};
    bool have_file = false, have_out = false;
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        if (a == "--help") return true;
        if (a == "--fresh" || a == "--reseed") {   // the flags without a value
            (a == "--fresh" ? p.fresh : p.reseed) = true;
            continue;
        }
        std::string key, val;
        bool has_val = false;
        if (a.size() > 1 && a[0] == '-') {
            std::string name = a;
            if (a.rfind("--", 0) == 0) {
                const size_t eq = a.find('=');
                if (eq != std::string::npos) {
                    name = a.substr(0, eq);
                    val = a.substr(eq + 1);
                    has_val = true;
                }
            } else if (a.size() > 2) {   // -n8
                name = a.substr(0, 2);
                val = a.substr(2);
                has_val = true;
            }
            const auto it = names.find(name);
            if (it == names.end()) throw std::invalid_argument("unrecognised option '" + a + "'");
            key = it->second;
            if (!has_val) {
                if (i + 1 >= argc) throw std::invalid_argument("the required argument for option '" + name + "' is missing");
                val = argv[++i];
            }
        } else {
            key = "file";   // positional
            val = a;
        }
        if (key == "n") p.n = parse_int(val, "-n");
        else if (key == "e") p.eps = std::stof(val);
        else if (key == "w") p.width = parse_int(val, "-w");
        else if (key == "h") p.height = parse_int(val, "-h");
        else if (key == "r") p.raport = parse_bool(val);
        else if (key == "q") p.quantizer = parse_int(val, "--quantizer");
        else if (key == "c") p.colorspace = parse_int(val, "--colorspace");
        else if (key == "device") setenv("QVQ_DEVICE", val.c_str(), 1);
        else if (key == "refine") {
            p.refine = parse_int(val, "--refine");
            if (p.refine < 0) throw std::invalid_argument("the argument ('" + val + "') for option '--refine' is invalid");
        }
        else if (key == "lloyd") {
            p.lloyd = parse_int(val, "--lloyd");
            if (p.lloyd < 0) throw std::invalid_argument("the argument ('" + val + "') for option '--lloyd' is invalid");
        }
        else if (key == "init") {
            if (val != "split" && val != "kmeans++" && val != "kmeans-par")
                throw std::invalid_argument("the argument ('" + val + "') for option '--init' is invalid");
            p.kmeanspp = val == "kmeans++";
            p.kmeanspar = val == "kmeans-par";
        }
        else if (key == "seed") {
            size_t pos = 0;
            if (val.empty() || val[0] == '-') pos = std::string::npos;
            else p.seed = std::stoull(val, &pos);
            if (pos != val.size()) throw std::invalid_argument("the argument ('" + val + "') for option '--seed' is invalid");
        }
        else if (key == "trials") {
            if (val.empty() || val[0] == '-' || val[0] == '+') throw std::invalid_argument("the argument ('" + val + "') for option '--trials' is invalid");
            p.trials = parse_int(val, "--trials");
            if (p.trials > 16) throw std::invalid_argument("the argument ('" + val + "') for option '--trials' is invalid");
        }
        else if (key == "o") {
            p.saveto = val;
            have_out = true;
        } else {
            if (have_file) throw std::invalid_argument("option '--file' cannot be specified more than once");
            p.file = val;
            have_file = true;
        }
    }
    if (!have_file) throw std::invalid_argument("the option '--file' is required but missing");
    if (!have_out) throw std::invalid_argument("the option '--saveto' is required but missing");
    if ((p.refine > 0 || p.fresh) && p.quantizer != (int)Quantizers::LBG)
        throw std::invalid_argument("options '--refine' and '--fresh' need the LBG quantizer");
    if (p.reseed && p.quantizer != (int)Quantizers::LBG)
        throw std::invalid_argument("option '--reseed' needs the LBG quantizer");
    if (p.lloyd > 0 && p.quantizer != (int)Quantizers::LBG)
        throw std::invalid_argument("option '--lloyd' needs the LBG quantizer");
    if (p.kmeanspp && p.quantizer != (int)Quantizers::LBG)
        throw std::invalid_argument("option '--init kmeans++' needs the LBG quantizer");
    if (p.kmeanspp && p.lloyd > 0)
        throw std::invalid_argument("option '--init kmeans++' cannot be combined with '--lloyd'");
    if (p.kmeanspar && p.quantizer != (int)Quantizers::LBG)
        throw std::invalid_argument("option '--init kmeans-par' needs the LBG quantizer");
    if (p.kmeanspar && p.lloyd > 0)
        throw std::invalid_argument("option '--init kmeans-par' cannot be combined with '--lloyd'");
    if (p.trials >= 0 && !p.kmeanspp)
        throw std::invalid_argument("option '--trials' needs '--init kmeans++'");
    if (p.reseed && p.refine <= 0 && p.lloyd <= 0)
        throw std::invalid_argument("option '--reseed' needs '--refine' > 0 or '--lloyd' > 0");
    return false;
}

}  // namespace

int main(int argc, char **argv) {
    Params par;
    try {
        if (parse(argc, argv, par)) {
            std::cout << kHelp << std::endl;
            return 0;
        }
    } catch (const std::exception &e) {
        std::cerr << "quant: " << e.what() << std::endl;
        std::cerr << "usage: quant FILE -o OUT [options]; quant --help lists them" << std::endl;
        return 2;
    }
    const FileType from = file_type(par.file), to = file_type(par.saveto);
    try {
        auto run_compression = [&]() {   // src/main.cpp:76-84
            RGBImage img(par.file);
            QuantizerPtr refined;
            if (par.kmeanspar) refined = getKMeansParQuantizer(par.seed, (size_t)par.refine, par.fresh, par.reseed);
            else if (par.kmeanspp && par.trials >= 0)
                refined = getGreedyKMeansPPQuantizer(par.seed, (unsigned)par.trials, (size_t)par.refine, par.fresh, par.reseed);
            else if (par.kmeanspp) refined = getKMeansPPQuantizer(par.seed, (size_t)par.refine, par.fresh, par.reseed);
            else if (par.lloyd > 0) refined = getLloydLBGQuantizer((size_t)par.lloyd, par.reseed, (size_t)par.refine, par.fresh);
            else if (par.refine > 0 || par.fresh) refined = getRefinedLBGQuantizer((size_t)par.refine, par.fresh, par.reseed);
            auto result = refined ? CompressedImage::compress(img, *refined, (ColorSpaces)par.colorspace, par.width,
                                                              par.height, par.eps, par.n)
                                  : CompressedImage::compress(img, (Quantizers)par.quantizer,
                                                              (ColorSpaces)par.colorspace, par.width, par.height,
                                                              par.eps, par.n);
            if (par.raport) std::cout << result.second;
            return result.first;
        };
        auto run_decompression = [&](const CompressedImage &c) {   // src/main.cpp:86-90
            RGBImage out = CompressedImage::decompress(c);
            out.saveToFile(par.saveto);
        };
        if (from == FileType::PPM && to == FileType::PPM) {
            run_decompression(run_compression());
        } else if (from == FileType::QUANT && to == FileType::PPM) {
            CompressedImage c;
            c.loadFromFile(par.file);
            run_decompression(c);
        } else if (from == FileType::PPM && to == FileType::QUANT) {
            CompressedImage c = run_compression();
            c.saveToFile(par.saveto);
        } else {
            std::cerr << "File type not supported" << std::endl;
            return 1;
        }
    } catch (const std::exception &e) {
        std::cerr << "quant: " << e.what() << std::endl;
        return 3;
    }
    return 0;
}
