// `path-tracer` command line — same surface as the reference binary for the
// render path (src/main.rs:14-57, src/config/mod.rs:10-52, README.md:28-60):
//
//   path-tracer render <INPUT> [-o/--output <OUTPUT>] [-q/--quiet] [-v/--viewer]
//                              [--debug-textures] [-p/--profile <PROFILE>] [--camera-path <CAMERAS>]
//                              [--keyframes <FRAMES> [--light-mixer]]
//                              [--denoise [--denoise-variance] [--denoise-guides <centre|samples>]] [--aov-dir <DIR>]
//                              [--noise-target <T> [--min-samples <N0>] [--max-samples <N>] [--noise-map <FILE.png>]
//                               [--adaptive [--adaptive-tile <N>] [--uniform-samples <U>] [--adaptive-dilate <0|1>]
//                                [--sample-map <FILE.png>]]
//                               [--film-denoise <plain|variance> [--filtered-target]]
//                               [--window-samples <W>]
//                               [--film-devices <A,B,..>]]
//                              [--temporal [--temporal-frames <H>] [--temporal-rotate <K>] [--temporal-normal-cos <C>]
//                               [--temporal-plane-tol <T>] [--temporal-map <FILE_%04d.png>]]
//       env OUTPUT (default render.png), env PROFILE
//   path-tracer convert <INPUT> <OUTPUT>      (glTF 2.0 -> ISF, host/gltf_convert.cpp)
//
// Any error prints the message on stderr and exits with code 2 (main.rs:14-22).
// The render itself runs on the GPU through the C ABI of include/ptgpu.h;
// there is no CPU fallback.  Extras (not in the reference): --device N,
// --devices A,B,... (one host thread per GPU, each rendering its share of interleaved 32x32 tiles: the
// sharding of SURVEY 8-e inside one process; the KD-tree and the origin grids are built once and uploaded to every
// device, the slices are exchanged by one RCCL all-gather), --stats (one JSON line with timings on stderr),
// --camera-path cams.json (a JSON array of ISF cameras: the scene is uploaded once and rendered from every camera in
// turn through pt_scene_set_camera; frame i goes to OUTPUT with i substituted for its one %d / %0Nd field),
// --keyframes frames.json (a JSON array of frames, each with any of a camera, all lights, material factor edits: the scene
// is uploaded once, frame i's edits are applied on top of frame i - 1's through pt_scene_set_camera / _set_lights /
// _set_materials, and frame i is written as with --camera-path), --light-mixer (with --keyframes: frames whose only edit
// is the colour of lights are mixed from the planes of one pt_lightmix capture instead of rendered),
// --noise-target T (every frame is a progressive film, pt_film_render_until: passes of N0, 2 N0, 4 N0, ... samples until the
// mean relative error of the pixels' mean luminance is <= T or the next pass would take the total above N),
// --adaptive (with --noise-target: an adaptive film, pt_film_render_until_adaptive - once every pixel has U samples the
// passes render only the N x N tiles whose mean error is still above T, and their neighbours; N bounds the largest count),
// --film-denoise (with --noise-target: the finished film goes through pt_film_denoise in place of pt_film_resolve) and
// --filtered-target (with --adaptive --film-denoise variance: pt_film_render_until_filtered - T is met by the filtered error),
// --window-samples W (with --noise-target: a windowed film, pt_film_render_until_windowed - windows of W samples of ONE
// enumeration of N = --max-samples samples, so the frame is a prefix of the render with samples = N and, run to its budget,
// that render byte for byte; T may be 0 here; --min-samples is refused, the first window has W samples),
// --film-devices A,B,.. (with --noise-target and --adaptive and/or --window-samples: the film is held by one shard film per entry
// - pt_film_create_shard, one host thread, scene and shard film each; the sharded loops exchange their tile noise through a
// barrier between the threads and take the same passes as the one-device loop; pt_film_assemble then makes the whole film on
// the first listed device and everything after the loop - resolve, filter, maps, PNG - runs on it unchanged: the same bytes),
// --temporal (with --camera-path or --keyframes: one pt_history for the run - every frame is rendered by pt_history_add_frame,
// joins the sums its pixels' surface points find in the previous view, and is written from the history: resolved, or with
// --denoise filtered by pt_history_denoise; max_samples = H x the profile's samples; a keyframe that edits lights or materials
// resets the history before its frame).
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <condition_variable>
#include <mutex>
#include <thread>
#include <sys/stat.h>
#include <unistd.h>
#include <utility>
#include <vector>

#include "ptgpu.h"
#include "pthost.h"

namespace {

[[noreturn]] void die(const std::string& msg) {
    fprintf(stderr, "%s\n", msg.c_str());
    exit(2);
}

void usage_render(FILE* f) {
    fputs("Path-trace awesome things\n\n"
          "Usage: path-tracer render [OPTIONS] <INPUT>\n\n"
          "Arguments:\n"
          "  <INPUT>  Input file name ISF format\n\n"
          "Options:\n"
          "  -o, --output <OUTPUT>    Output image name [env: OUTPUT=] [default: render.png]\n"
          "  -q, --quiet              No progress bar printed\n"
          "  -v, --viewer             Display a viewer (headless: the output file is refreshed after every sample batch)\n"
          "      --debug-textures     Generate debug textures\n"
          "  -p, --profile <PROFILE>  A path to the yaml file containing all the rendering profile information [env: PROFILE=]\n"
          "      --device <N>         HIP device ordinal [default: 0]\n"
          "      --devices <A,B,..>   Render on several GPUs (interleaved tiles, one thread per device)\n"
          "      --stats              Print timing statistics as JSON on stderr\n"
          "      --camera-path <CAMERAS>  Render one frame per camera of a JSON array of ISF cameras; the OUTPUT name\n"
          "                           takes the frame index in its %d / %0Nd field (e.g. out/frame_%04d.png)\n"
          "      --keyframes <FRAMES>  Render one frame per object of a JSON array of keyframes (\"camera\", \"lights\",\n"
          "                           \"materials\" edits, each frame on top of the last); OUTPUT as with --camera-path\n"
          "      --light-mixer        With --keyframes: capture light-mixer planes where the next frame changes light colours only\n"
          "                           and mix such frames from them instead of rendering (one device, not with --denoise)\n"
          "      --denoise            Write the frame filtered by the edge-avoiding a-trous denoiser (first-hit normal, depth and\n"
          "                           albedo guides); one device only, -v previews stay raw\n"
          "      --denoise-iterations <N>  Filter passes of --denoise, pass i has step 2^i [0..8, default: the library's]\n"
          "      --denoise-variance   With --denoise: steer the filter's colour weight by the per-pixel variance of the frame's own\n"
          "                           samples (needs samples >= 2 in the profile)\n"
          "      --denoise-guides <centre|samples>  With --denoise: the guides of the pixel-centre ray's first hit, or the mean features\n"
          "                           of the surfaces the frame's own samples shaded (their camera casts and alpha walks replayed)\n"
          "                           [default: centre; samples: not with --noise-target]\n"
          "      --aov-dir <DIR>      Write albedo.png, normal.png, depth.png and alpha.png of the frame's samples into DIR (created);\n"
          "                           a single frame on one device (not with --camera-path, --keyframes, --noise-target or --devices)\n"
          "      --noise-target <T>   Progressive film: add passes of N0, 2 N0, 4 N0, ... samples until the mean relative error of\n"
          "                           the pixels' mean luminance is <= T or the next pass would exceed N samples in all (one\n"
          "                           device, not with --light-mixer; -v prints one line per pass)\n"
          "      --min-samples <N0>   First pass of --noise-target [>= 2, default: 8]\n"
          "      --max-samples <N>    Sample budget of --noise-target [default: the profile's samples]\n"
          "      --noise-map <FILE.png>  With --noise-target: write the per-pixel error as grey, white = 2 T and above\n"
          "      --adaptive           With --noise-target: later passes render only the tiles whose mean error is above T; the run\n"
          "                           ends when no tile is, or at N samples in the busiest pixel (not with --denoise)\n"
          "      --adaptive-tile <N>  Tile size of --adaptive [a multiple of 8 with N*N a multiple of 256, default: 32]\n"
          "      --uniform-samples <U>  Every pass of --adaptive is a whole frame until every pixel has U samples [default: 24]\n"
          "      --adaptive-dilate <0|1>  --adaptive also renders the 8 neighbours of a tile above T [default: 1]\n"
          "      --sample-map <FILE.png>  With --adaptive: write the per-pixel sample count as grey, white = the largest\n"
          "      --film-denoise <plain|variance>  With --noise-target: write the finished film, uniform or adaptive, filtered on the\n"
          "                           device by the a-trous denoiser with every pixel's own sample count (--denoise-iterations\n"
          "                           applies; one device, not with --denoise)\n"
          "      --window-samples <W> With --noise-target: a windowed film - every pass adds the next W samples of ONE enumeration of\n"
          "                           N = --max-samples samples (the active tiles only, with --adaptive), so the frame is a prefix of\n"
          "                           the render with samples = N, and exactly that render when it runs to its budget; T may be 0\n"
          "                           [>= 2; not with --min-samples or --filtered-target]\n"
          "      --film-devices <A,B,..>  With --noise-target and --adaptive and/or --window-samples: the film's tiles are shared by one\n"
          "                           shard film per listed device (repeats allowed), the loop runs on all of them in lock-step and\n"
          "                           the whole film is assembled on the first; the output is the one-device run's, byte for byte\n"
          "      --filtered-target    With --adaptive --film-denoise variance: T is met by the error of the FILTERED image - tiles\n"
          "                           are selected by the variance the filter leaves; --noise-map then shows that error\n"
          "      --temporal           With --camera-path or --keyframes: keep a temporal history along the path - every frame's\n"
          "                           samples join those its pixels' surface points find in the previous view (a static scene; a\n"
          "                           keyframe that edits lights or materials starts the history afresh); with --denoise the\n"
          "                           history is filtered with every pixel's own sample count (one device)\n"
          "      --temporal-frames <H>  The history of a pixel is capped at H frames' samples [default: 4]\n"
          "      --temporal-rotate <K>  Frame i renders the samples [jN, jN + N), j = i mod K, of an enumeration of K N samples, so\n"
          "                           that still pixels do not see the same samples again [default: the library's]\n"
          "      --temporal-normal-cos <C>  The least cosine between the normals of a pixel and its history [default: the library's]\n"
          "      --temporal-plane-tol <T>  The largest distance of the history's point from the pixel's plane, relative to its depth\n"
          "                           [default: the library's]\n"
          "      --temporal-map <FILE_%04d.png>  Write where every pixel's history came from as grey: white a source, black no\n"
          "                           surface, the greys between: outside the previous view, then the test that failed\n"
          "  -h, --help               Print help\n",
          f);
}

void usage_main(FILE* f) {
    fputs("Path-trace awesome things\n\n"
          "Usage: path-tracer <COMMAND>\n\n"
          "Commands:\n"
          "  render   Path-trace awesome things\n"
          "  convert  Convert scenes into ISF format\n"
          "  help     Print this message or the help of the given subcommand(s)\n\n"
          "Options:\n"
          "  -h, --help     Print help\n"
          "  -V, --version  Print version\n",
          f);
}

struct Progress {
    bool quiet;
    std::chrono::steady_clock::time_point start;
};

// -v / --viewer on a headless node: the viewer feed (renderer/mod.rs:133-141, renderer/viewer.rs) becomes a
// progressively refreshed output file — after every sample batch the image of the samples done so far.
struct Preview {
    std::string path;
    uint32_t width, height;
};
void on_preview(const uint8_t* rgb8, uint64_t n_pixels, uint32_t, uint32_t, void* user) {
    Preview* v = (Preview*)user;
    if (n_pixels == (uint64_t)v->width * v->height) pth_png_write_rgb8(v->path.c_str(), v->width, v->height, rgb8);
}

// The one %d / %0Nd field of an output name: (prefix, zero-pad width, suffix).  false: no field; a malformed or second
// field is an error.
bool frame_pattern(const std::string& out, std::string& pre, int& width, std::string& post) {
    size_t at = std::string::npos;
    for (size_t i = 0; i < out.size(); ++i) {
        if (out[i] != '%') continue;
        if (at != std::string::npos) die("error: the output name '" + out + "' has more than one % field (one %d or %0Nd expected)");
        at = i;
    }
    if (at == std::string::npos) return false;
    size_t j = at + 1;
    width = 0;
    if (j < out.size() && out[j] == '0') {
        ++j;
        size_t k = j;
        while (j < out.size() && isdigit((unsigned char)out[j])) ++j;
        if (j == k) die("error: the output name '" + out + "' has a malformed % field (%d or %0Nd expected)");
        width = atoi(out.substr(k, j - k).c_str());
    }
    if (j >= out.size() || out[j] != 'd' || width > 32) die("error: the output name '" + out + "' has a malformed % field (%d or %0Nd expected)");
    pre = out.substr(0, at);
    post = out.substr(j + 1);
    return true;
}

// --noise-target with -v: one line per pass
void on_film_pass(const pt_film_info* info, const pt_film_noise_stats* noise, void* user) {
    if (!*(const bool*)user) return;
    fprintf(stderr, "film: pass %u: %u samples (%llu in all), noise %.6g, over target %.4f of the blocks\n", info->passes,
            info->last_pass_samples, (unsigned long long)info->samples, noise->mean_error, noise->fraction_over);
}

// --noise-target --adaptive with -v: one line per pass
struct AdaptivePassCtx {
    bool verbose;
    pt_film* film;
};
void on_adaptive_pass(const pt_film_info* info, const pt_film_noise_stats* noise, void* user) {
    const AdaptivePassCtx* ctx = (const AdaptivePassCtx*)user;
    if (!ctx->verbose) return;
    pt_film_adaptive_info ai{};
    if (pt_film_get_adaptive_info(ctx->film, &ai) != PT_OK) return;
    fprintf(stderr, "film: pass %u: %u samples, %u of %u tiles, noise %.6g\n", info->passes, info->last_pass_samples,
            ai.last_pass_tiles, ai.n_tiles, noise->mean_error);
}

// A whole non-negative decimal number that fits 32 bits, or die.
uint32_t parse_u32(const std::string& v, const char* name) {
    if (v.empty() || v.size() > 9 || v.find_first_not_of("0123456789") != std::string::npos)
        die("error: invalid value '" + v + "' for '" + name + "': a whole number expected");
    return (uint32_t)strtoul(v.c_str(), nullptr, 10);
}

void on_progress(uint32_t done, uint32_t total, void* user) {
    Progress* p = (Progress*)user;
    if (p->quiet) return;
    int width = 40, filled = total ? (int)((uint64_t)done * width / total) : width;
    fprintf(stderr, "\rRendering: %u / %u [", done, total);
    for (int i = 0; i < width; ++i) fputc(i < filled ? '=' : (i == filled ? '>' : '-'), stderr);
    fprintf(stderr, "] %3u %%", total ? (unsigned)((uint64_t)done * 100 / total) : 100u);
    fflush(stderr);
}

int run_render(int argc, char** argv) {
    std::string input, output, profile_path;
    std::string camera_path, keyframes_path;
    bool have_output = false, have_profile = false, quiet = false, debug_textures = false, stats = false, viewer = false;
    bool have_camera_path = false, have_keyframes = false;
    bool denoise = false, denoise_variance = false, light_mixer = false;
    int denoise_iterations = -1;
    bool have_noise_target = false, have_min_samples = false, have_max_samples = false;
    double noise_target = 0.0;
    uint32_t min_samples = 8, max_samples = 0;
    std::string noise_map, sample_map;
    bool adaptive = false, have_adaptive_tile = false, have_uniform_samples = false, have_adaptive_dilate = false;
    uint32_t adaptive_tile = 32, uniform_samples = 0, adaptive_dilate = 1;
    std::string film_denoise;   // "", "plain" or "variance"
    std::string denoise_guides; // "", "centre" or "samples"
    std::string aov_dir;
    bool filtered_target = false;
    bool have_window_samples = false;
    uint32_t window_samples = 0;
    std::string noise_target_text;
    int device = 0;
    std::vector<int> devices, film_devices;
    bool have_film_devices = false;
    bool temporal = false, have_temporal_frames = false, have_temporal_rotate = false;
    uint32_t temporal_frames = 4, temporal_rotate = 0;
    std::string temporal_normal_cos, temporal_plane_tol, temporal_map;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        auto value = [&](const char* name) -> std::string {
            size_t eq = a.find('=');
            if (a.rfind("--", 0) == 0 && eq != std::string::npos) return a.substr(eq + 1);
            if (i + 1 >= argc) die(std::string("error: a value is required for '") + name + "' but none was supplied");
            return argv[++i];
        };
        if (a == "-h" || a == "--help") {
            usage_render(stdout);
            return 0;
        } else if (a == "-o" || a == "--output" || a.rfind("--output=", 0) == 0) {
            output = value("--output <OUTPUT>");
            have_output = true;
        } else if (a.rfind("-o", 0) == 0 && a.size() > 2 && a[1] == 'o') {
            output = a.substr(2);
            have_output = true;
        } else if (a == "-p" || a == "--profile" || a.rfind("--profile=", 0) == 0) {
            profile_path = value("--profile <PROFILE>");
            have_profile = true;
        } else if (a.rfind("-p", 0) == 0 && a.size() > 2 && a[1] == 'p') {
            profile_path = a.substr(2);
            have_profile = true;
        } else if (a == "-q" || a == "--quiet") quiet = true;
        else if (a == "-v" || a == "--viewer") viewer = true;  // no window system here: progressive output file
        else if (a == "-qv" || a == "-vq") quiet = viewer = true;
        else if (a == "--debug-textures") debug_textures = true;
        else if (a == "--stats") stats = true;
        else if (a == "--denoise") denoise = true;
        else if (a == "--light-mixer") light_mixer = true;
        else if (a == "--temporal") temporal = true;
        else if (a == "--temporal-frames" || a.rfind("--temporal-frames=", 0) == 0) {
            temporal_frames = parse_u32(value("--temporal-frames <H>"), "--temporal-frames <H>");
            have_temporal_frames = true;
        } else if (a == "--temporal-rotate" || a.rfind("--temporal-rotate=", 0) == 0) {
            temporal_rotate = parse_u32(value("--temporal-rotate <K>"), "--temporal-rotate <K>");
            have_temporal_rotate = true;
        } else if (a == "--temporal-normal-cos" || a.rfind("--temporal-normal-cos=", 0) == 0)
            temporal_normal_cos = value("--temporal-normal-cos <C>");
        else if (a == "--temporal-plane-tol" || a.rfind("--temporal-plane-tol=", 0) == 0)
            temporal_plane_tol = value("--temporal-plane-tol <T>");
        else if (a == "--temporal-map" || a.rfind("--temporal-map=", 0) == 0) temporal_map = value("--temporal-map <FILE_%04d.png>");
        else if (a == "--denoise-variance") denoise_variance = true;
        else if (a == "--denoise-iterations" || a.rfind("--denoise-iterations=", 0) == 0) {
            std::string v = value("--denoise-iterations <N>");
            if (v.empty() || v.size() > 1 || !isdigit((unsigned char)v[0]) || v[0] > '8')
                die("error: invalid value '" + v + "' for '--denoise-iterations <N>': 0..8 expected");
            denoise_iterations = v[0] - '0';
        }
        else if (a == "--denoise-guides" || a.rfind("--denoise-guides=", 0) == 0) {
            denoise_guides = value("--denoise-guides <centre|samples>");
            if (denoise_guides != "centre" && denoise_guides != "samples")
                die("error: invalid value '" + denoise_guides + "' for '--denoise-guides <centre|samples>': centre or samples expected");
        } else if (a == "--aov-dir" || a.rfind("--aov-dir=", 0) == 0) {
            aov_dir = value("--aov-dir <DIR>");
            if (aov_dir.empty()) die("error: invalid value '' for '--aov-dir <DIR>': a directory name expected");
        }
        else if (a == "--noise-target" || a.rfind("--noise-target=", 0) == 0) {
            std::string v = value("--noise-target <T>");
            char* end = nullptr;
            noise_target = strtod(v.c_str(), &end);
            // (zero is a target only a windowed film takes - render the whole enumeration: checked once every flag is known)
            if (v.empty() || *end || !(noise_target >= 0.0) || !std::isfinite(noise_target))
                die("error: invalid value '" + v + "' for '--noise-target <T>': a positive, finite number expected");
            noise_target_text = v;
            have_noise_target = true;
        } else if (a == "--min-samples" || a.rfind("--min-samples=", 0) == 0) {
            min_samples = parse_u32(value("--min-samples <N0>"), "--min-samples <N0>");
            have_min_samples = true;
        } else if (a == "--max-samples" || a.rfind("--max-samples=", 0) == 0) {
            max_samples = parse_u32(value("--max-samples <N>"), "--max-samples <N>");
            have_max_samples = true;
        } else if (a == "--noise-map" || a.rfind("--noise-map=", 0) == 0) noise_map = value("--noise-map <FILE.png>");
        else if (a == "--adaptive") adaptive = true;
        else if (a == "--film-denoise" || a.rfind("--film-denoise=", 0) == 0) {
            film_denoise = value("--film-denoise <plain|variance>");
            if (film_denoise != "plain" && film_denoise != "variance")
                die("error: invalid value '" + film_denoise + "' for '--film-denoise <plain|variance>': plain or variance expected");
        } else if (a == "--filtered-target") filtered_target = true;
        else if (a == "--window-samples" || a.rfind("--window-samples=", 0) == 0) {
            window_samples = parse_u32(value("--window-samples <W>"), "--window-samples <W>");
            have_window_samples = true;
        }
        else if (a == "--adaptive-tile" || a.rfind("--adaptive-tile=", 0) == 0) {
            adaptive_tile = parse_u32(value("--adaptive-tile <N>"), "--adaptive-tile <N>");
            have_adaptive_tile = true;
        } else if (a == "--uniform-samples" || a.rfind("--uniform-samples=", 0) == 0) {
            uniform_samples = parse_u32(value("--uniform-samples <U>"), "--uniform-samples <U>");
            have_uniform_samples = true;
        } else if (a == "--adaptive-dilate" || a.rfind("--adaptive-dilate=", 0) == 0) {
            std::string v = value("--adaptive-dilate <0|1>");
            if (v != "0" && v != "1") die("error: invalid value '" + v + "' for '--adaptive-dilate <0|1>': 0 or 1 expected");
            adaptive_dilate = v == "1" ? 1u : 0u;
            have_adaptive_dilate = true;
        } else if (a == "--sample-map" || a.rfind("--sample-map=", 0) == 0) sample_map = value("--sample-map <FILE.png>");
        else if (a == "--camera-path" || a.rfind("--camera-path=", 0) == 0) {
            camera_path = value("--camera-path <CAMERAS>");
            have_camera_path = true;
        } else if (a == "--keyframes" || a.rfind("--keyframes=", 0) == 0) {
            keyframes_path = value("--keyframes <FRAMES>");
            have_keyframes = true;
        }
        else if (a == "--devices" || a.rfind("--devices=", 0) == 0) {
            std::string list = value("--devices <A,B,..>");
            devices.clear();
            for (size_t p = 0; p <= list.size();) {
                size_t q = list.find(',', p);
                if (q == std::string::npos) q = list.size();
                if (q == p) die("error: invalid value '" + list + "' for '--devices <A,B,..>'");
                devices.push_back(atoi(list.substr(p, q - p).c_str()));
                p = q + 1;
            }
        } else if (a == "--film-devices" || a.rfind("--film-devices=", 0) == 0) {
            std::string list = value("--film-devices <A,B,..>");
            film_devices.clear();
            have_film_devices = true;
            for (size_t p = 0; p <= list.size();) {
                size_t q = list.find(',', p);
                if (q == std::string::npos) q = list.size();
                const std::string item = list.substr(p, q - p);
                if (item.empty() || item.size() > 4 || item.find_first_not_of("0123456789") != std::string::npos)
                    die("error: invalid value '" + list + "' for '--film-devices <A,B,..>': a list of device ordinals expected");
                film_devices.push_back(atoi(item.c_str()));
                p = q + 1;
            }
        } else if (a == "--device" || a.rfind("--device=", 0) == 0) device = atoi(value("--device <N>").c_str());
        else if (a.size() > 1 && a[0] == '-' && a != "-")
            die("error: unexpected argument '" + a + "' found\n\nUsage: path-tracer render [OPTIONS] <INPUT>");
        else if (input.empty()) input = a;
        else die("error: unexpected argument '" + a + "' found\n\nUsage: path-tracer render [OPTIONS] <INPUT>");
    }
    if (input.empty()) die("error: the following required arguments were not provided:\n  <INPUT>\n\nUsage: path-tracer render [OPTIONS] <INPUT>");
    if (!have_output) {
        const char* e = getenv("OUTPUT");
        output = e && *e ? e : "render.png";
    }
    if (!have_profile) {
        const char* e = getenv("PROFILE");
        if (e && *e) {
            profile_path = e;
            have_profile = true;
        }
    }

    if (have_film_devices) {
        auto with = [](const char* other, const char* why) {
            die(std::string("error: the argument '--film-devices <A,B,..>' cannot be used with '") + other + "' (" + why + ")");
        };
        if (!have_noise_target) die("error: '--film-devices <A,B,..>' needs '--noise-target <T>'");
        if (!adaptive && !have_window_samples)
            die("error: '--film-devices <A,B,..>' needs '--adaptive' or '--window-samples <W>' (a sharded film is measured tile by tile)");
        if (!devices.empty()) with("--devices <A,B,..>", "one list of devices per run");
        if (filtered_target) with("--filtered-target", "the filter needs the whole image in every pass");
        if (denoise) with("--denoise", "the finished film is filtered by '--film-denoise <plain|variance>'");
        if (light_mixer) with("--light-mixer", "mixed frames have no samples to add to");
        if (have_camera_path) with("--camera-path <CAMERAS>", "a sharded film renders one frame");
        if (have_keyframes) with("--keyframes <FRAMES>", "a sharded film renders one frame");
        device = film_devices[0];   // the whole film is assembled, resolved and filtered there
    }
    pt_history_params hist_params;
    pt_history_params_default(&hist_params);
    if (!temporal && (have_temporal_frames || have_temporal_rotate || !temporal_normal_cos.empty() || !temporal_plane_tol.empty() ||
                      !temporal_map.empty()))
        die("error: '--temporal-frames <H>', '--temporal-rotate <K>', '--temporal-normal-cos <C>', '--temporal-plane-tol <T>' and "
            "'--temporal-map <FILE_%04d.png>' need '--temporal'");
    if (temporal) {
        auto with = [](const char* other, const char* why) {
            die(std::string("error: the argument '--temporal' cannot be used with '") + other + "' (" + why + ")");
        };
        if (!have_camera_path && !have_keyframes) die("error: '--temporal' needs '--camera-path <CAMERAS>' or '--keyframes <FRAMES>'");
        if (have_noise_target) with("--noise-target <T>", "a film adds samples to one view, a history carries them between views");
        if (!film_denoise.empty()) with("--film-denoise <plain|variance>", "the history is filtered by '--denoise'");
        if (have_film_devices) with("--film-devices <A,B,..>", "a history lives on one device");
        if (light_mixer) with("--light-mixer", "mixed frames have no samples to add to");
        if (!aov_dir.empty()) with("--aov-dir <DIR>", "the planes are written for a single frame");
        if (!denoise_guides.empty()) with("--denoise-guides <centre|samples>", "a history is filtered with the guides of its own samples");
        if (devices.size() > 1) with("--devices <A,B,..>", "a history lives on one device");
        if (debug_textures) with("--debug-textures", "debug textures are one frame without samples");
        auto number = [](const std::string& v, const char* name, float lo, float hi) {
            char* end = nullptr;
            const float x = strtof(v.c_str(), &end);
            if (v.empty() || *end || !(x >= lo && x <= hi))
                die("error: invalid value '" + v + "' for '" + name + "': a number in " + std::to_string(lo) + " .. " + std::to_string(hi) + " expected");
            return x;
        };
        if (!temporal_normal_cos.empty()) hist_params.normal_cos = number(temporal_normal_cos, "--temporal-normal-cos <C>", -1.f, 1.f);
        if (!temporal_plane_tol.empty()) hist_params.plane_tol = number(temporal_plane_tol, "--temporal-plane-tol <T>", 0.f, 1e6f);
        if (have_temporal_rotate) {
            if (temporal_rotate < 1 || temporal_rotate > 4096)
                die("error: invalid value '" + std::to_string(temporal_rotate) + "' for '--temporal-rotate <K>': 1 .. 4096 expected");
            hist_params.rotate = temporal_rotate;
        }
        if (temporal_frames < 1)
            die("error: invalid value '" + std::to_string(temporal_frames) + "' for '--temporal-frames <H>': at least 1");
        if (!temporal_map.empty()) {
            std::string ext = temporal_map.size() >= 4 ? temporal_map.substr(temporal_map.size() - 4) : "";
            for (char& c : ext) c = (char)tolower(c);
            if (ext != ".png") die("The image format could not be determined (only .png output is supported): " + temporal_map);
        }
    }
    if (denoise_iterations >= 0 && !denoise && film_denoise.empty()) die("error: '--denoise-iterations <N>' needs '--denoise'");
    if (denoise_variance && !denoise) die("error: '--denoise-variance' needs '--denoise'");
    if (!denoise_guides.empty() && !film_denoise.empty())
        die("error: the argument '--denoise-guides <centre|samples>' cannot be used with '--film-denoise <plain|variance>' (a film's "
            "pixels have sample counts of their own)");
    if (!denoise_guides.empty() && !denoise) die("error: '--denoise-guides <centre|samples>' needs '--denoise'");
    if (denoise_guides == "samples" && have_noise_target)
        die("error: the argument '--denoise-guides samples' cannot be used with '--noise-target <T>' (a film's pixels have sample "
            "counts of their own)");
    if (!aov_dir.empty()) {
        auto with = [](const char* other, const char* why) {
            die(std::string("error: the argument '--aov-dir <DIR>' cannot be used with '") + other + "' (" + why + ")");
        };
        if (have_camera_path) with("--camera-path <CAMERAS>", "the planes are written for a single frame");
        if (have_keyframes) with("--keyframes <FRAMES>", "the planes are written for a single frame");
        if (have_noise_target) with("--noise-target <T>", "a film's pixels have sample counts of their own");
        if (devices.size() > 1) with("--devices <A,B,..>", "the planes are made on one device");
        if (debug_textures) with("--debug-textures", "one set of feature images per run");
    }
    if (denoise && devices.size() > 1)
        die("error: the argument '--denoise' cannot be used with more than one device in '--devices <A,B,..>' (the gathered "
            "multi-GPU frame is u8 only; the filter needs the f32 frame on one device)");
    if (light_mixer && !have_keyframes) die("error: '--light-mixer' needs '--keyframes <FRAMES>'");
    if (light_mixer && denoise) die("error: the argument '--light-mixer' cannot be used with '--denoise' (mixed frames are not filtered)");
    if (light_mixer && devices.size() > 1)
        die("error: the argument '--light-mixer' cannot be used with more than one device in '--devices <A,B,..>' (mixed frames "
            "are not gathered)");
    if (!have_noise_target && (have_min_samples || have_max_samples || !noise_map.empty()))
        die("error: '--min-samples <N0>', '--max-samples <N>' and '--noise-map <FILE.png>' need '--noise-target <T>'");
    if (have_noise_target && !have_window_samples && !(noise_target > 0.0 && (float)noise_target > 0.f))
        die("error: invalid value '" + noise_target_text + "' for '--noise-target <T>': a positive, finite number expected");
    if (have_window_samples && !have_noise_target) die("error: '--window-samples <W>' needs '--noise-target <T>'");
    if (have_window_samples && window_samples < 2)
        die("error: invalid value '" + std::to_string(window_samples) + "' for '--window-samples <W>': at least 2 (a sample variance needs two samples)");
    if (have_window_samples && have_min_samples)
        die("error: the argument '--window-samples <W>' cannot be used with '--min-samples <N0>' (the first window has W samples)");
    if (have_window_samples && filtered_target)
        die("error: the argument '--window-samples <W>' cannot be used with '--filtered-target' (the filtered selection is not built "
            "for windows)");
    if (adaptive && !have_noise_target) die("error: '--adaptive' needs '--noise-target <T>'");
    if (!adaptive && (have_adaptive_tile || have_uniform_samples || have_adaptive_dilate || !sample_map.empty()))
        die("error: '--adaptive-tile <N>', '--uniform-samples <U>', '--adaptive-dilate <0|1>' and '--sample-map <FILE.png>' need "
            "'--noise-target <T> --adaptive'");
    if (adaptive && denoise)
        die("error: the argument '--adaptive' cannot be used with '--denoise' or '--denoise-variance' (the filters take one sample "
            "count for the whole frame)");
    if (!film_denoise.empty() && !have_noise_target) die("error: '--film-denoise <plain|variance>' needs '--noise-target <T>'");
    if (!film_denoise.empty() && denoise)
        die("error: the argument '--film-denoise <plain|variance>' cannot be used with '--denoise' (one filter per frame)");
    if (!film_denoise.empty() && devices.size() > 1)
        die("error: the argument '--film-denoise <plain|variance>' cannot be used with more than one device in '--devices <A,B,..>' "
            "(the filter needs the whole film on one device)");
    if (filtered_target && film_denoise == "plain")
        die("error: the argument '--filtered-target' cannot be used with '--film-denoise plain' (the plain filter carries no variance)");
    if (filtered_target && (!adaptive || film_denoise.empty())) die("error: '--filtered-target' needs '--adaptive --film-denoise variance'");
    if (adaptive && devices.size() > 1)
        die("error: the argument '--adaptive' cannot be used with more than one device in '--devices <A,B,..>' (an adaptive film "
            "lives on one device)");
    if (adaptive && (adaptive_tile == 0 || adaptive_tile > 4096 || (adaptive_tile & 7u) || ((adaptive_tile * adaptive_tile) & 255u)))
        die("error: invalid value '" + std::to_string(adaptive_tile) + "' for '--adaptive-tile <N>': a multiple of 8 with N*N a multiple of 256 expected");
    if (!sample_map.empty()) {
        std::string ext = sample_map.size() >= 4 ? sample_map.substr(sample_map.size() - 4) : "";
        for (char& c : ext) c = (char)tolower(c);
        if (ext != ".png") die("The image format could not be determined (only .png output is supported): " + sample_map);
    }
    if (have_noise_target && light_mixer)
        die("error: the argument '--noise-target <T>' cannot be used with '--light-mixer' (mixed frames have no samples to add to)");
    if (have_noise_target && devices.size() > 1)
        die("error: the argument '--noise-target <T>' cannot be used with more than one device in '--devices <A,B,..>' (the noise "
            "figure is taken over the whole image on one device)");
    if (have_noise_target && debug_textures) die("error: the argument '--noise-target <T>' cannot be used with '--debug-textures'");
    if (!noise_map.empty()) {
        std::string ext = noise_map.size() >= 4 ? noise_map.substr(noise_map.size() - 4) : "";
        for (char& c : ext) c = (char)tolower(c);
        if (ext != ".png") die("The image format could not be determined (only .png output is supported): " + noise_map);
    }

    // Profile::load / Default (main.rs:33-36)
    pt_profile profile;
    if (pth_profile_load(have_profile ? profile_path.c_str() : nullptr, &profile) != PT_OK) die(pth_last_error());
    if (have_noise_target) {
        if (!have_max_samples) max_samples = profile.samples;
        if (have_window_samples) {
            if (max_samples < 2)
                die("error: '--window-samples <W>' needs an enumeration of at least 2 samples ('--max-samples <N>' or the profile's samples: " +
                    std::to_string(max_samples) + ")");
            min_samples = 2;   // (not a parameter of the windowed loop; keeps the checks below quiet)
        }
        if (min_samples < 2)
            die("error: invalid value '" + std::to_string(min_samples) + "' for '--min-samples <N0>': at least 2 (a sample variance needs two samples)");
        if (min_samples > max_samples)
            die("error: '--min-samples <N0>' (" + std::to_string(min_samples) + ") exceeds the sample budget (" + std::to_string(max_samples) +
                ": '--max-samples <N>' or the profile's samples)");
        if (max_samples > (uint32_t)PT_FILM_MAX_SAMPLES)
            die("error: invalid value '" + std::to_string(max_samples) + "' for '--max-samples <N>': at most " + std::to_string((uint32_t)PT_FILM_MAX_SAMPLES));
    }
    if (temporal) {
        const uint64_t cap = (uint64_t)temporal_frames * profile.samples;
        if (profile.samples < 1 || cap + profile.samples > (uint64_t)PT_FILM_MAX_SAMPLES ||
            (uint64_t)hist_params.rotate * profile.samples > (uint64_t)PT_FILM_MAX_SAMPLES)
            die("error: '--temporal-frames <H>' (" + std::to_string(temporal_frames) + ") and '--temporal-rotate <K>' (" +
                std::to_string(hist_params.rotate) + ") times the profile's samples (" + std::to_string(profile.samples) +
                ") must stay below " + std::to_string((uint32_t)PT_FILM_MAX_SAMPLES));
        hist_params.max_samples = (uint32_t)cap;
    }
    if (denoise_variance && !have_noise_target && profile.samples < 2)
        die("error: '--denoise-variance' needs a profile with samples >= 2 (a sample variance of " + std::to_string(profile.samples) +
            " sample does not exist)");

    // --camera-path / --keyframes: everything they can get wrong is found before any GPU work
    std::vector<pt_camera> cameras;
    pth_keyframe* keyframes = nullptr;
    uint32_t n_keyframes = 0;
    std::string out_pre, out_post;
    int out_width = 0;
    bool out_field = false;
    if (have_camera_path && have_keyframes) die("error: the argument '--keyframes <FRAMES>' cannot be used with '--camera-path <CAMERAS>'");
    if (have_camera_path || have_keyframes) {
        const char* opt = have_camera_path ? "--camera-path <CAMERAS>" : "--keyframes <FRAMES>";
        if (debug_textures) die(std::string("error: the argument '--debug-textures' cannot be used with '") + opt + "'");
        size_t n_frames = 0;
        if (have_camera_path) {
            pt_camera* cams = nullptr;
            uint32_t n_cams = 0;
            if (pth_camera_path_load(camera_path.c_str(), &cams, &n_cams) != PT_OK) die(pth_last_error());
            cameras.assign(cams, cams + n_cams);
            pth_camera_path_free(cams);
            n_frames = cameras.size();
        } else {
            if (pth_keyframes_load(keyframes_path.c_str(), &keyframes, &n_keyframes) != PT_OK) die(pth_last_error());
            n_frames = n_keyframes;
        }
        out_field = frame_pattern(output, out_pre, out_width, out_post);
        if (n_frames > 1 && !out_field)
            die(std::string("error: ") + (have_camera_path ? "--camera-path" : "--keyframes") + " has " + std::to_string(n_frames) +
                (have_camera_path ? " cameras" : " frames") + " but the output name '" + output + "' has no %d / %0Nd field for the frame index");
        size_t dot = output.find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : output.substr(dot + 1);
        for (char& c : ext) c = (char)tolower(c);
        if (ext != "png") die("The image format could not be determined (only .png output is supported): " + output);
    }
    auto frame_name = [&](size_t f) {
        if (!out_field) return output;
        char num[48];
        snprintf(num, sizeof num, "%0*zu", out_width, f);
        return out_pre + num + out_post;
    };
    std::string map_pre, map_post;
    int map_width = 0;
    bool map_field = false;
    if (!temporal_map.empty()) {
        map_field = frame_pattern(temporal_map, map_pre, map_width, map_post);
        if ((have_camera_path ? cameras.size() : (size_t)n_keyframes) > 1 && !map_field)
            die("error: the name '" + temporal_map + "' of '--temporal-map <FILE_%04d.png>' has no %d / %0Nd field for the frame index");
    }
    auto map_name = [&](size_t f) {
        if (!map_field) return temporal_map;
        char num[48];
        snprintf(num, sizeof num, "%0*zu", map_width, f);
        return map_pre + num + map_post;
    };

    auto t0 = std::chrono::steady_clock::now();
    pth_scene* hscene = nullptr;  // load_internal (main.rs:38)
    if (pth_scene_load_isf(input.c_str(), &hscene) != PT_OK) die(pth_last_error());
    // What every frame after the first changes (--camera-path: its camera; --keyframes: the state its edits leave), found
    // by applying the frames to the host scene in turn - a material index out of range ends the run here, before any GPU
    // work - and the host scene left in frame 0's state for pt_scene_create (frame 0: no grid rebuild).
    struct FrameEdit {
        bool camera = false, lights = false, materials = false;
        pt_camera cam{};
        std::vector<pt_light> light;
        std::vector<pt_material> material;
    };
    std::vector<FrameEdit> edits;
    for (const pt_camera& c : cameras) {
        edits.emplace_back();
        edits.back().camera = true;
        edits.back().cam = c;
    }
    if (keyframes) {
        auto snapshot = [&](FrameEdit& e) {
            const pt_scene_desc* d = pth_scene_desc(hscene);
            e.cam = d->camera;
            e.light.assign(d->lights, d->lights + d->n_lights);
            e.material.assign(d->materials, d->materials + d->n_materials);
        };
        for (uint32_t f = 0; f < n_keyframes; ++f) {
            if (pth_keyframe_apply(hscene, &keyframes[f]) != PT_OK) die(std::string("frame ") + std::to_string(f) + ": " + pth_last_error());
            edits.emplace_back();
            FrameEdit& e = edits.back();
            e.camera = keyframes[f].has_camera != 0;
            e.lights = keyframes[f].has_lights != 0;
            e.materials = keyframes[f].n_materials > 0;
            snapshot(e);
        }
        const FrameEdit& e0 = edits[0];
        if (pth_scene_set_camera(hscene, &e0.cam) != PT_OK || pth_scene_set_lights(hscene, e0.light.data(), (uint32_t)e0.light.size()) != PT_OK ||
            pth_scene_set_materials(hscene, e0.material.data(), (uint32_t)e0.material.size()) != PT_OK)
            die(pth_last_error());
        pth_keyframes_free(keyframes);
        keyframes = nullptr;
    } else if (!cameras.empty() && pth_scene_set_camera(hscene, &cameras[0]) != PT_OK) {
        die(pth_last_error());
    }
    // frame f's edits on a device's scene (f > 0)
    auto apply_frame = [&](pt_scene* sc, size_t f) {
        const FrameEdit& e = edits[f];
        int rc = PT_OK;
        if (e.camera) rc = pt_scene_set_camera(sc, &e.cam);
        if (rc == PT_OK && e.lights) rc = pt_scene_set_lights(sc, e.light.data(), (uint32_t)e.light.size());
        if (rc == PT_OK && e.materials) rc = pt_scene_set_materials(sc, e.material.data(), (uint32_t)e.material.size());
        return rc;
    };
    auto t1 = std::chrono::steady_clock::now();

    if (devices.size() == 1 || (debug_textures && !devices.empty())) {
        device = devices[0];
        devices.clear();
    }
    pt_scene* scene = nullptr;   // (several devices: every worker thread creates its own below)
    if (devices.empty() && pt_scene_create(pth_scene_desc(hscene), device, &scene) != PT_OK) die(pt_last_error());
    auto t2 = std::chrono::steady_clock::now();

    if (debug_textures) {  // debug_render(&scene, profile.resolution); return (main.rs:40-43)
        static const char* names[PT_DEBUG_PLANES] = {"normal", "albedo", "opacity", "metalness", "roughness", "emissive", "ior"};
        size_t plane = (size_t)profile.width * profile.height * 3;
        std::vector<uint8_t> planes(plane * PT_DEBUG_PLANES);
        int any_hit = 0;
        if (pt_debug_render(scene, profile.width, profile.height, planes.data(), &any_hit) != PT_OK) die(pt_last_error());
        if (any_hit)  // the reference creates the buffers on the first hit: no hit, no files
            for (int p = 0; p < PT_DEBUG_PLANES; ++p)
                if (pth_png_write_rgb8((std::string(names[p]) + ".png").c_str(), profile.width, profile.height,
                                       planes.data() + plane * p) != PT_OK)
                    die(pth_last_error());
        pt_scene_destroy(scene);
        pth_scene_free(hscene);
        return 0;
    }

    if (devices.size() > 1) {
        // One host thread per GPU.  The host work (KD-tree, origin grids) is done ONCE (pt_prep) and uploaded to every
        // device; tile (tx, ty) of the 32x32 grid goes to shard (tx + ty * s) mod N (diagonal stripes, pt_local_pixel_map;
        // the global pixel index stays in the RNG seed, so the assembled image equals the single-GPU one bit for bit).
        // Distinct devices exchange their packed u8 slices with one RCCL all-gather over xGMI and scatter them on the
        // device (pt_gather_tiles); a device list with repeats (several shards on one GPU: a rehearsal) is assembled on
        // the host, RCCL does not allow duplicates.
        // Two phases with a barrier between them: every worker uploads its scene first, and the collective phase is
        // entered only if ALL of them succeeded - a worker that failed would never arrive at the all-gather and the
        // others would wait for it forever.  A failure INSIDE the collective phase (after the peers may already be
        // enqueued in ncclAllGather) ends the process with the message and exit code 2 instead of joining.
        const uint32_t n = (uint32_t)devices.size();
        pt_prep* prep = nullptr;
        if (pt_prep_create(pth_scene_desc(hscene), &prep) != PT_OK) die(pt_last_error());
        bool distinct = true;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = i + 1; j < n; ++j)
                if (devices[i] == devices[j]) distinct = false;
        std::vector<pt_comm*> comms(n, nullptr);
        if (distinct && pt_comm_create_all(devices.data(), (int)n, comms.data()) != PT_OK) die(pt_last_error());
        uint64_t slice_pixels = 0;
        std::vector<pt_opts> opts(n);
        for (uint32_t k = 0; k < n; ++k) {
            memset(&opts[k], 0, sizeof(pt_opts));
            opts[k].device = devices[k];
            opts[k].shard_rank = k;
            opts[k].shard_count = n;
            opts[k].tile_w = opts[k].tile_h = 32;
            slice_pixels = std::max<uint64_t>(slice_pixels, pt_local_pixel_count(&profile, &opts[k]));
        }
        const size_t n_frames = edits.empty() ? 1 : edits.size();   // (--camera-path / --keyframes: every scene takes every frame)
        std::vector<std::vector<std::vector<uint8_t>>> part(n, std::vector<std::vector<uint8_t>>(n_frames));
        std::vector<std::vector<uint32_t>> map(n);
        std::vector<std::string> error(n);
        std::vector<std::vector<uint8_t>> frames(n_frames, std::vector<uint8_t>((size_t)profile.width * profile.height * 3));
        std::mutex bar_mutex;
        std::condition_variable bar_cv;
        uint32_t arrived = 0, failed = 0;
        auto worker = [&](uint32_t k) {
            pt_scene* sc = nullptr;
            auto check = [&](int rc) {   // (the message is thread-local: read it on this thread)
                if (rc != PT_OK && error[k].empty()) error[k] = pt_last_error();
                return rc == PT_OK;
            };
            const bool up = check(pt_scene_create_from_prep(prep, devices[k], &sc));
            {   // barrier: all scenes are resident, or nobody renders
                std::unique_lock<std::mutex> lock(bar_mutex);
                if (!up) ++failed;
                if (++arrived == n) bar_cv.notify_all();
                else bar_cv.wait(lock, [&] { return arrived == n; });
            }
            for (size_t f = 0; f < n_frames && up && failed == 0 && error[k].empty(); ++f) {
                if (distinct) {
                    if ((f > 0 && !check(apply_frame(sc, f))) ||
                        !check(pt_render_gathered(sc, comms[k], &profile, &opts[k], slice_pixels, k == 0 ? frames[f].data() : nullptr))) {
                        fprintf(stderr, "Error: %s\n", error[k].c_str());   // (the peers may be inside the all-gather: do not join them)
                        fflush(stderr);
                        _exit(2);
                    }
                } else {
                    if (f > 0 && !check(apply_frame(sc, f))) break;
                    uint64_t count = pt_local_pixel_count(&profile, &opts[k]);
                    map[k].resize(count);
                    part[k][f].resize(count * 3);
                    if (check(pt_local_pixel_map(&profile, &opts[k], map[k].data())))
                        check(pt_render(sc, &profile, &opts[k], part[k][f].data(), nullptr));
                }
            }
            if (sc) pt_scene_destroy(sc);
        };
        std::vector<std::thread> threads;
        for (uint32_t k = 0; k < n; ++k) threads.emplace_back(worker, k);
        for (auto& t : threads) t.join();
        for (pt_comm* c : comms) pt_comm_destroy(c);
        pt_prep_destroy(prep);
        for (uint32_t k = 0; k < n; ++k)
            if (!error[k].empty()) die(error[k]);
        if (!distinct)
            for (size_t f = 0; f < n_frames; ++f)
                for (uint32_t k = 0; k < n; ++k)
                    for (size_t i = 0; i < map[k].size(); ++i) memcpy(&frames[f][(size_t)map[k][i] * 3], &part[k][f][i * 3], 3);
        auto t3 = std::chrono::steady_clock::now();
        if (!quiet)
            fprintf(stderr, "Done: %llds\n", (long long)std::chrono::duration_cast<std::chrono::seconds>(t3 - t2).count());
        size_t dot = output.find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : output.substr(dot + 1);
        for (char& c : ext) c = (char)tolower(c);
        if (ext != "png") die("The image format could not be determined (only .png output is supported): " + output);
        for (size_t f = 0; f < n_frames; ++f)
            if (pth_png_write_rgb8(frame_name(f).c_str(), profile.width, profile.height, frames[f].data()) != PT_OK) die(pth_last_error());
        if (stats) {
            double sec = std::chrono::duration<double>(t3 - t2).count();
            fprintf(stderr, "{\"devices\": %u, \"gather\": \"%s\", \"render_s\": %.3f, \"msamples_per_s\": %.2f}\n", n,
                    distinct ? "rccl" : "host", sec, (double)profile.width * profile.height * profile.samples / sec / 1e6);
        }
        pth_scene_free(hscene);
        return 0;
    }

    // Renderer::new + render (main.rs:46-47)
    Progress prog{quiet, std::chrono::steady_clock::now()};
    pt_opts opts;
    memset(&opts, 0, sizeof opts);
    opts.device = device;
    opts.flags = PT_FLAG_TIMING;
    if (!quiet) {
        opts.progress = on_progress;
        opts.progress_user = &prog;
    }
    if (!quiet || viewer) opts.sample_batch = profile.samples > 16 ? (profile.samples + 15) / 16 : 1;  // ~16 ticks
    Preview pv{output, profile.width, profile.height};
    if (viewer) {
        size_t dot = output.find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : output.substr(dot + 1);
        if (ext == "png" || ext == "PNG") {
            opts.preview = on_preview;
            opts.preview_user = &pv;
        }
    }
    std::vector<uint8_t> rgb((size_t)profile.width * profile.height * 3);
    pt_denoise_params dn;
    if (denoise_variance || film_denoise == "variance") pt_denoise_var_params_default(&dn);
    else pt_denoise_params_default(&dn);
    dn.tonemap = profile.tonemap;
    if (denoise_iterations >= 0) dn.iterations = (uint32_t)denoise_iterations;
    const size_t n_frames = edits.empty() ? 1 : edits.size();   // (--camera-path / --keyframes: one frame each, the scene kept)
    auto t3 = t2, t4 = t2;
    // --light-mixer: frame f is colour-only when its keyframe has no camera and no materials and its lights are the previous
    // state's in count, kind, vec and size.  A capture lives until the first frame that is not; while it lives the scene is
    // not told about the colours (lights_of: the frame whose lights it has), so a mixed frame costs no grid rebuild.
    auto colour_only = [&](size_t f) {
        return f > 0 && f < n_frames && !edits[f].camera && !edits[f].materials &&
               pth_lights_differ_in_color_only(edits[f - 1].light.data(), (uint32_t)edits[f - 1].light.size(), edits[f].light.data(),
                                               (uint32_t)edits[f].light.size());
    };
    // --noise-target: one film for the run; every frame starts it from zero passes
    pt_film* film = nullptr;
    pt_opts film_opts = opts;
    if (adaptive) film_opts.tile_w = film_opts.tile_h = adaptive_tile;   // (the film's tiling is what its passes select by)
    pt_profile film_profile = profile;
    if (have_window_samples) film_profile.samples = max_samples;   // the enumeration
    if (have_noise_target && (have_window_samples ? pt_film_create_windowed(device, &film_profile, &film_opts, &film)
                                                  : pt_film_create(device, &profile, &film_opts, &film)) != PT_OK)
        die(pt_last_error());
    const size_t n_pixels = (size_t)profile.width * profile.height;
    // one frame's map, grey: the frame index goes in front of the extension when there are several
    auto write_map = [&](const std::string& map, size_t f, const std::vector<uint8_t>& grey) {
        std::string name = map;
        if (n_frames > 1) {
            char num[32];
            snprintf(num, sizeof num, "_%zu", f);
            name = map.substr(0, map.size() - 4) + num + map.substr(map.size() - 4);
        }
        if (pth_png_write_rgb8(name.c_str(), profile.width, profile.height, grey.data()) != PT_OK) die(pth_last_error());
    };
    auto to_grey = [](float v) { return (uint8_t)(!(v == v) || v <= 0.f ? 0 : (v >= 255.f ? 255 : (uint8_t)v)); };
    // --film-devices: one thread, scene and shard film per entry, the host work done once (pt_prep).  Two phases, as with
    // --devices: every worker makes its scene and its shard film first, and the loop - whose exchange is a barrier between the
    // workers - is entered only if ALL of them succeeded.  A failure inside the loop (the peers may be waiting in the barrier)
    // ends the process with the message and exit code 2.  Then the shards are assembled into `film`.
    struct FilmExchange {
        std::mutex m;
        std::condition_variable cv;
        uint32_t n = 0, arrived = 0, generation = 0;
        std::vector<float> acc_sum, acc_max, out_sum, out_max;
        // every entry is its owner's value or +0.f, and errors are not negative: the largest is the owner's, bit for bit
        static int call(float* tile_sum, float* tile_max, uint32_t n_tiles, void* user) {
            FilmExchange& x = *(FilmExchange*)user;
            std::unique_lock<std::mutex> lock(x.m);
            if (x.arrived == 0) {
                x.acc_sum.assign(n_tiles, 0.f);
                x.acc_max.assign(n_tiles, 0.f);
            }
            if (x.acc_sum.size() != n_tiles) return 1;
            for (uint32_t i = 0; i < n_tiles; ++i) {
                if (tile_sum[i] > x.acc_sum[i]) x.acc_sum[i] = tile_sum[i];
                if (tile_max[i] > x.acc_max[i]) x.acc_max[i] = tile_max[i];
            }
            if (++x.arrived == x.n) {
                x.out_sum = x.acc_sum;
                x.out_max = x.acc_max;
                x.arrived = 0;
                ++x.generation;
                x.cv.notify_all();
            } else {
                const uint32_t g = x.generation;
                x.cv.wait(lock, [&] { return x.generation != g; });
            }
            memcpy(tile_sum, x.out_sum.data(), n_tiles * sizeof(float));
            memcpy(tile_max, x.out_max.data(), n_tiles * sizeof(float));
            return 0;
        }
    };
    auto render_film_sharded = [&](pt_film_tile_stats& tiles) {
        const uint32_t n = (uint32_t)film_devices.size();
        pt_prep* prep = nullptr;
        if (pt_prep_create(pth_scene_desc(hscene), &prep) != PT_OK) die(pt_last_error());
        std::vector<pt_film*> shards(n, nullptr);
        std::vector<std::string> error(n);
        std::vector<pt_film_tile_stats> outs(n);
        FilmExchange exchange;
        exchange.n = n;
        std::mutex bar_mutex;
        std::condition_variable bar_cv;
        uint32_t arrived = 0, failed = 0;
        auto worker = [&](uint32_t k) {
            pt_scene* sc = nullptr;
            auto check = [&](int rc) {   // (the message is thread-local: read it on this thread)
                if (rc != PT_OK && error[k].empty()) error[k] = pt_last_error();
                return rc == PT_OK;
            };
            pt_opts o = film_opts;
            o.device = film_devices[k];
            o.shard_rank = k;
            o.shard_count = n;
            o.progress = nullptr;
            o.preview = nullptr;
            const bool up = check(pt_scene_create_from_prep(prep, film_devices[k], &sc)) &&
                            check(pt_film_create_shard(film_devices[k], &film_profile, &o, have_window_samples ? 1u : 0u, &shards[k]));
            {   // barrier: all scenes and shard films are resident, or nobody enters the loop
                std::unique_lock<std::mutex> lock(bar_mutex);
                if (!up) ++failed;
                if (++arrived == n) bar_cv.notify_all();
                else bar_cv.wait(lock, [&] { return arrived == n; });
            }
            if (up && failed == 0) {
                AdaptivePassCtx ctx{viewer && k == 0, shards[k]};   // (every rank sees the same passes: rank 0 prints them)
                int rc;
                if (have_window_samples) {
                    pt_film_window_params wp;
                    pt_film_window_params_default(&wp);
                    wp.target = noise_target;
                    wp.window_samples = window_samples;
                    wp.adaptive = adaptive ? 1u : 0u;
                    if (have_uniform_samples) wp.uniform_samples = uniform_samples;
                    if (have_adaptive_dilate) wp.dilate = adaptive_dilate;
                    rc = pt_film_render_until_windowed_sharded(shards[k], sc, &wp, FilmExchange::call, &exchange, on_adaptive_pass, &ctx, &outs[k]);
                } else {
                    pt_film_adaptive_params ap;
                    pt_film_adaptive_params_default(&ap);
                    ap.target = noise_target;
                    ap.first_pass_samples = min_samples;
                    ap.max_samples = max_samples;
                    if (have_uniform_samples) ap.uniform_samples = uniform_samples;
                    if (have_adaptive_dilate) ap.dilate = adaptive_dilate;
                    rc = pt_film_render_until_adaptive_sharded(shards[k], sc, &ap, FilmExchange::call, &exchange, on_adaptive_pass, &ctx, &outs[k]);
                }
                if (!check(rc)) {
                    fprintf(stderr, "Error: %s\n", error[k].c_str());   // (the peers may be inside the exchange: do not join them)
                    fflush(stderr);
                    _exit(2);
                }
            }
            if (sc) pt_scene_destroy(sc);
        };
        std::vector<std::thread> threads;
        for (uint32_t k = 0; k < n; ++k) threads.emplace_back(worker, k);
        for (auto& t : threads) t.join();
        pt_prep_destroy(prep);
        for (uint32_t k = 0; k < n; ++k)
            if (!error[k].empty()) die(error[k]);
        if (pt_film_assemble(film, shards.data(), n) != PT_OK) die(pt_last_error());
        for (pt_film* s : shards) pt_film_destroy(s);
        tiles = outs[0];
    };
    auto render_film = [&](size_t f) {
        if (f > 0 && pt_film_reset(film) != PT_OK) die(pt_last_error());
        pt_film_noise_stats noise{};
        pt_film_tile_stats tiles{};
        if (have_film_devices) {
            render_film_sharded(tiles);
            noise.mean_error = tiles.mean_error;
            noise.converged = tiles.converged;
        } else if (have_window_samples) {
            pt_film_window_params wp;
            pt_film_window_params_default(&wp);
            wp.target = noise_target;
            wp.window_samples = window_samples;
            wp.adaptive = adaptive ? 1u : 0u;
            if (have_uniform_samples) wp.uniform_samples = uniform_samples;
            if (have_adaptive_dilate) wp.dilate = adaptive_dilate;
            AdaptivePassCtx ctx{viewer, film};
            if (pt_film_render_until_windowed(film, scene, &wp, on_adaptive_pass, &ctx, &tiles) != PT_OK) die(pt_last_error());
            noise.mean_error = tiles.mean_error;
            noise.converged = tiles.converged;
        } else if (adaptive) {
            pt_film_adaptive_params ap;
            pt_film_adaptive_params_default(&ap);
            ap.target = noise_target;
            ap.first_pass_samples = min_samples;
            ap.max_samples = max_samples;
            if (have_uniform_samples) ap.uniform_samples = uniform_samples;
            if (have_adaptive_dilate) ap.dilate = adaptive_dilate;
            AdaptivePassCtx ctx{viewer, film};
            if (filtered_target) {   // tiles are selected by the error of the filtered image
                pt_film_filtered_params fp;
                fp.adaptive = ap;
                fp.filter = dn;
                if (pt_film_render_until_filtered(film, scene, &fp, on_adaptive_pass, &ctx, &tiles) != PT_OK) die(pt_last_error());
            } else if (pt_film_render_until_adaptive(film, scene, &ap, on_adaptive_pass, &ctx, &tiles) != PT_OK) {
                die(pt_last_error());
            }
            noise.mean_error = tiles.mean_error;
            noise.converged = tiles.converged;
        } else if (pt_film_render_until(film, scene, min_samples, max_samples, PT_FILM_DEFAULT_LUM_FLOOR, noise_target, on_film_pass,
                                        &viewer, &noise) != PT_OK) {
            die(pt_last_error());
        }
        pt_film_info info{};
        if (pt_film_get_info(film, &info) != PT_OK) die(pt_last_error());
        if (denoise) {   // the film's planes through the filter, samples = the film's total
            std::vector<float> acc(n_pixels * 3), mom(n_pixels * 2), guides(n_pixels * PT_GUIDE_FLOATS);
            if (pt_film_read(film, acc.data(), mom.data()) != PT_OK || pt_render_guides(scene, profile.width, profile.height, guides.data()) != PT_OK)
                die(pt_last_error());
            if ((denoise_variance ? pt_denoise_var(device, profile.width, profile.height, (uint32_t)info.samples, &dn, acc.data(), mom.data(),
                                                   guides.data(), nullptr, rgb.data())
                                  : pt_denoise(device, profile.width, profile.height, (uint32_t)info.samples, &dn, acc.data(), guides.data(),
                                               nullptr, rgb.data())) != PT_OK)
                die(pt_last_error());
        } else if (!film_denoise.empty()) {   // the film's own planes through the filter on the device, every pixel by its count
            if (pt_film_denoise(film, scene, film_denoise == "variance", &dn, PT_FILM_DEFAULT_LUM_FLOOR, rgb.data(), nullptr, nullptr) != PT_OK)
                die(pt_last_error());
        } else if (pt_film_resolve(film, profile.tonemap, rgb.data(), nullptr) != PT_OK) {
            die(pt_last_error());
        }
        if (!noise_map.empty()) {   // grey = as_u8(min(1, err / (2 T)) * 255)
            std::vector<float> err(n_pixels);
            if ((filtered_target ? pt_film_filtered_noise(film, scene, &dn, PT_FILM_DEFAULT_LUM_FLOOR, noise_target, &tiles, err.data(), nullptr, nullptr)
                 : adaptive || have_window_samples ? pt_film_tile_noise(film, PT_FILM_DEFAULT_LUM_FLOOR, noise_target, &tiles, err.data(), nullptr, nullptr)
                                 : pt_film_noise(film, PT_FILM_DEFAULT_LUM_FLOOR, noise_target, &noise, err.data(), nullptr, nullptr)) != PT_OK)
                die(pt_last_error());
            std::vector<uint8_t> grey(n_pixels * 3);
            const float full = 2.0f * (float)noise_target;
            for (size_t i = 0; i < n_pixels; ++i) grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = to_grey(fminf(1.0f, err[i] / full) * 255.0f);
            write_map(noise_map, f, grey);
        }
        if (!sample_map.empty()) {   // grey = as_u8(count / max_count * 255)
            std::vector<uint32_t> counts(n_pixels);
            if (pt_film_read_counts(film, counts.data()) != PT_OK) die(pt_last_error());
            std::vector<uint8_t> grey(n_pixels * 3);
            for (size_t i = 0; i < n_pixels; ++i)
                grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = to_grey((float)counts[i] / (float)info.samples * 255.0f);
            write_map(sample_map, f, grey);
        }
        if (adaptive || have_window_samples)
            fprintf(stderr, "film: %u passes, %llu samples, %s %.6g, %s, pixel-samples %llu of %llu\n", info.passes,
                    (unsigned long long)info.samples, filtered_target ? "filtered noise" : "noise", noise.mean_error,
                    noise.converged ? "converged" : "max samples",
                    (unsigned long long)tiles.pixel_samples, (unsigned long long)(info.n_local * info.samples));
        else
            fprintf(stderr, "film: %u passes, %llu samples, noise %.6g, %s\n", info.passes, (unsigned long long)info.samples, noise.mean_error,
                    noise.converged ? "converged" : "max samples");
    };
    // --aov-dir: the frame's pixel records (pt_render_aov) as four images in the debug pass's conventions, as_u8(v * 255):
    // albedo = sum / N, normal = the normalised sum * 0.5 + 0.5, depth = (sum / coverage) over the largest finite one,
    // alpha = coverage / N; a pixel without coverage stays 0 in all of them
    auto write_aov_planes = [&]() {
        std::vector<float> aov(n_pixels * PT_AOV_FLOATS);
        if (pt_render_aov(scene, &profile, &opts, 0u, aov.data()) != PT_OK) die(pt_last_error());
        for (size_t p = 1; p <= aov_dir.size(); ++p)
            if (p == aov_dir.size() || aov_dir[p] == '/') (void)mkdir(aov_dir.substr(0, p).c_str(), 0777);   // (existing: fine)
        const float fn = (float)profile.samples;
        float zmax = 0.f;
        for (size_t i = 0; i < n_pixels; ++i) {
            const float* r = &aov[i * PT_AOV_FLOATS];
            const float z = r[3] / r[7];
            if (r[7] > 0.f && std::isfinite(z) && z > zmax) zmax = z;
        }
        std::vector<uint8_t> albedo(n_pixels * 3, 0), normal(n_pixels * 3, 0), depth(n_pixels * 3, 0), alpha(n_pixels * 3, 0);
        for (size_t i = 0; i < n_pixels; ++i) {
            const float* r = &aov[i * PT_AOV_FLOATS];
            if (!(r[7] > 0.f)) continue;
            const float nn = (r[0] * r[0] + r[1] * r[1]) + r[2] * r[2];
            const float inv = nn > 0.f && nn < INFINITY ? 1.0f / sqrtf(nn) : 0.f;
            for (int c = 0; c < 3; ++c) {
                albedo[3 * i + c] = to_grey((r[4 + c] / fn) * 255.0f);
                normal[3 * i + c] = to_grey(((r[c] * inv) * 0.5f + 0.5f) * 255.0f);
                depth[3 * i + c] = to_grey(((r[3] / r[7]) / zmax) * 255.0f);
                alpha[3 * i + c] = to_grey((r[7] / fn) * 255.0f);
            }
        }
        const std::pair<const char*, const std::vector<uint8_t>*> files[] = {
            {"albedo.png", &albedo}, {"normal.png", &normal}, {"depth.png", &depth}, {"alpha.png", &alpha}};
        for (const auto& file : files)
            if (pth_png_write_rgb8((aov_dir + "/" + file.first).c_str(), profile.width, profile.height, file.second->data()) != PT_OK)
                die(pth_last_error());
    };
    // --temporal: one history for the run
    pt_history* hist = nullptr;
    if (temporal && pt_history_create(device, profile.width, profile.height, &hist_params, &hist) != PT_OK) die(pt_last_error());
    auto render_temporal = [&](size_t f) {
        if (f > 0 && (edits[f].lights || edits[f].materials) && pt_history_reset(hist) != PT_OK) die(pt_last_error());
        if (pt_history_add_frame(hist, scene, &profile, &opts, (uint32_t)f) != PT_OK) die(pt_last_error());
        if ((denoise ? pt_history_denoise(hist, denoise_variance ? 1 : 0, &dn, PT_FILM_DEFAULT_LUM_FLOOR, rgb.data(), nullptr)
                     : pt_history_resolve(hist, profile.tonemap, rgb.data(), nullptr)) != PT_OK)
            die(pt_last_error());
        if (temporal_map.empty()) return;
        std::vector<int32_t> src(n_pixels);
        if (pt_history_read(hist, nullptr, nullptr, nullptr, nullptr, nullptr, src.data()) != PT_OK) die(pt_last_error());
        std::vector<uint8_t> grey(n_pixels * 3);
        for (size_t i = 0; i < n_pixels; ++i) {   // -1 black, -2 .. -6: 32, 64, 96, 128, 160, a source: white
            const uint8_t g = src[i] >= 0 ? 255 : (uint8_t)(32 * (-src[i] - 1));
            grey[3 * i] = grey[3 * i + 1] = grey[3 * i + 2] = g;
        }
        if (pth_png_write_rgb8(map_name(f).c_str(), profile.width, profile.height, grey.data()) != PT_OK) die(pth_last_error());
    };
    pt_lightmix* mix = nullptr;
    bool mixer_on = light_mixer;
    size_t lights_of = 0, captures = 0, mixed = 0, rendered = 0;
    for (size_t f = 0; f < n_frames; ++f) {
        bool use_mix = false;
        if (light_mixer) {
            if (mix && !colour_only(f)) {
                pt_lightmix_destroy(mix);
                mix = nullptr;
            }
            if (f > 0 && !mix) {   // the scene takes the frame; its lights also when earlier mixed frames held them back
                FrameEdit& e = edits[f];
                e.lights = e.lights || lights_of != f - 1;
                if (apply_frame(scene, f) != PT_OK) die(pt_last_error());
                lights_of = f;
            }
            if (!mix && mixer_on && colour_only(f + 1)) {
                const int rc = pt_lightmix_capture(scene, &profile, &opts, &mix);
                if (rc == PT_ERR_UNSUPPORTED) mixer_on = false;   // (more lights than a capture takes: every frame is rendered)
                else if (rc != PT_OK) die(pt_last_error());
                else ++captures;
            }
            use_mix = mix != nullptr;
        } else if (f > 0 && apply_frame(scene, f) != PT_OK) die(pt_last_error());
        pv.path = frame_name(f);
        if (use_mix) {
            std::vector<float> colors;
            for (const pt_light& l : edits[f].light) colors.insert(colors.end(), l.color, l.color + 3);
            if (pt_lightmix_apply(mix, colors.data(), profile.tonemap, rgb.data(), nullptr) != PT_OK) die(pt_last_error());
            ++mixed;
        } else if (film) {
            render_film(f);
            ++rendered;
        } else if (hist) {
            render_temporal(f);
            ++rendered;
        } else {
            if ((denoise_guides == "samples"
                     ? pt_render_denoised_aov(scene, &profile, &opts, &dn, denoise_variance ? 1 : 0, 0u, rgb.data(), nullptr)
                 : denoise_variance ? pt_render_denoised_var(scene, &profile, &opts, &dn, rgb.data(), nullptr)
                 : denoise        ? pt_render_denoised(scene, &profile, &opts, &dn, rgb.data(), nullptr)
                                  : pt_render(scene, &profile, &opts, rgb.data(), nullptr)) != PT_OK)
                die(pt_last_error());
            ++rendered;
        }
        t3 = std::chrono::steady_clock::now();
        if (!quiet)
            fprintf(stderr, "\nDone: %llds\n", (long long)std::chrono::duration_cast<std::chrono::seconds>(t3 - t2).count());

        // rendered_image.save(output) (main.rs:50); the format follows the extension, PNG only here
        size_t dot = output.find_last_of('.');
        std::string ext = dot == std::string::npos ? "" : output.substr(dot + 1);
        for (char& c : ext) c = (char)tolower(c);
        if (ext != "png") die("The image format could not be determined (only .png output is supported): " + output);
        if (pth_png_write_rgb8(frame_name(f).c_str(), profile.width, profile.height, rgb.data()) != PT_OK) die(pth_last_error());
        if (!aov_dir.empty()) write_aov_planes();
        t4 = std::chrono::steady_clock::now();
    }

    if (mix) pt_lightmix_destroy(mix);
    if (film) pt_film_destroy(film);
    if (hist) pt_history_destroy(hist);
    if (light_mixer) fprintf(stderr, "light mixer: %zu captures, %zu mixed frames, %zu rendered frames\n", captures, mixed, rendered);

    if (stats) {
        pt_timing tm{};
        pt_scene_info info{};
        pt_get_timing(scene, &tm);
        pt_scene_get_info(scene, &info);
        auto sec = [](auto a, auto b) { return std::chrono::duration<double>(b - a).count(); };
        double samples = (double)profile.width * profile.height * profile.samples * n_frames;
        fprintf(stderr,
                // load = ISF + textures; build = pt_scene_create (KD-tree and origin grids side by side on the host, upload);
                // render = pt_render (kernels + the copy back); png = the output file
                "{\"load_s\": %.3f, \"build_s\": %.3f, \"kd_build_s\": %.3f, \"grid_build_s\": %.3f, \"upload_s\": %.3f, "
                "\"render_s\": %.3f, \"kernel_ms\": %.3f, \"png_s\": %.3f, \"total_s\": %.3f, \"msamples_per_s\": %.2f, "
                "\"prims\": %llu, \"kd_nodes\": %llu, \"leaf_refs\": %llu, \"cam_grid_res\": %u, \"light_grids\": %u%s}\n",
                sec(t0, t1), sec(t1, t2), (double)info.kd_build_seconds, (double)info.grid_build_seconds, (double)info.upload_seconds,
                sec(t2, t3), (double)tm.integrate_ms, sec(t3, t4), sec(t0, t4), samples / sec(t2, t3) / 1e6,
                (unsigned long long)info.n_prims, (unsigned long long)info.n_kd_nodes, (unsigned long long)info.n_leaf_refs,
                info.cam_grid_res, info.light_grids,
                have_film_devices ? (", \"film_devices\": " + std::to_string(film_devices.size())).c_str() : "");
    }
    pt_scene_destroy(scene);
    pth_scene_free(hscene);
    return 0;
}

// path-tracer convert <INPUT> <OUTPUT> (config/mod.rs:44-52, main.rs:54-57)
int run_convert(int argc, char** argv) {
    std::vector<std::string> pos;
    for (int i = 0; i < argc; ++i) {
        std::string a = argv[i];
        if (a == "-h" || a == "--help") {
            fputs("Convert scenes into ISF format\n\n"
                  "Usage: path-tracer convert <INPUT> <OUTPUT>\n\n"
                  "Arguments:\n"
                  "  <INPUT>   Input file name gltf format\n"
                  "  <OUTPUT>  Output directory name\n\n"
                  "Options:\n"
                  "  -h, --help  Print help\n",
                  stdout);
            return 0;
        }
        if (a.size() > 1 && a[0] == '-') die("error: unexpected argument '" + a + "' found\n\nUsage: path-tracer convert <INPUT> <OUTPUT>");
        pos.push_back(a);
    }
    if (pos.size() < 2)
        die(std::string("error: the following required arguments were not provided:\n") + (pos.empty() ? "  <INPUT>\n" : "") +
            "  <OUTPUT>\n\nUsage: path-tracer convert <INPUT> <OUTPUT>");
    if (pos.size() > 2) die("error: unexpected argument '" + pos[2] + "' found\n\nUsage: path-tracer convert <INPUT> <OUTPUT>");
    if (pth_convert_gltf(pos[0].c_str(), pos[1].c_str()) != PT_OK) die(pth_last_error());
    return 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        usage_main(stderr);
        return 2;
    }
    std::string cmd = argv[1];
    if (cmd == "render") return run_render(argc - 2, argv + 2);
    if (cmd == "convert") return run_convert(argc - 2, argv + 2);
    if (cmd == "-h" || cmd == "--help" || cmd == "help") {
        usage_main(stdout);
        return 0;
    }
    if (cmd == "-V" || cmd == "--version") {
        printf("path-tracer 0.1.0 (%s)\n", pt_version());
        return 0;
    }
    die("error: unrecognized subcommand '" + cmd + "'\n\nUsage: path-tracer <COMMAND>");
}
