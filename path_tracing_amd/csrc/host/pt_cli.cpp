// pt_cli -- dependency-free clone of the reference's headless front-end for the PT path
// (reference src/main_cli.cpp:42-256): same flags, same banner, same scene grammar, same
// camera (FOV hard-coded to 50 like the reference, main_cli.cpp:158), same 8-bit output stage;
// PNG through zlib instead of OpenCV.  Extra flags the reference lacks:
//   --width/--height  override the scene's R line        --seed N   reproducible streams
//   --max-depth N     eye depth (reference: EYE_DEPTH 4)  --obj FILE append an OBJ's faces (current material: 0.7 grey diffuse)
//   --rr              optional unbiased Russian roulette (pt)
//   --gpus N          render on N devices of this node inside the blocking call (image tiles, RCCL gather)
//   --radius R        photon search radius of --mode ppm, initial radius of --mode sppm (reference: PPM_RADIUS 0.05)
//   --alpha A         radius reduction of --mode sppm (default 0.7)
//   --denoise         filter the frame before it is saved: --guide-spp N guide samples (default 4), then the edge-avoiding
//                     a-trous filter (--denoise-iterations, --sigma-color, --sigma-normal, --sigma-position; 0 = default)
//   --frames N        progressive: N frames of --frame-spp S samples (default: --spp; ppm: passes), frame f with sample offset
//                     f * S, accumulated and presented on the device; --rms-log FILE gets "<frame> <rms>" per frame (the
//                     reference GUI's RMS history, src/main.cpp:502-530), --until-rms R stops after a frame >= 2 whose rms <= R.
//                     The PNG holds the last presented bytes.  pt, bdpt and ppm on one device.
//   --orbit DEG       with --frames: frame f renders from the scene's eye rotated by f * DEG degrees about the look-at point
//                     around the up vector (rotation in double, rounded to float, then the usual camera).  By itself it does
//                     what the reference's GUI does when the camera moves: the accumulation restarts on every moved frame.
//   --spin DEG        with --frames and --obj: frame f turns the OBJ's triangles by f * DEG degrees about the vertical axis
//                     through their centroid and updates the live scene; --reproject follows them (the motion guide)
//   --spin-device DEG --spin through hpt_scene_set_parts once and hpt_scene_pose per frame: the OBJ is one rigid part, the host
//                     hands over twelve floats per frame and copies no record; not together with --spin
//   --twist-device DEG with --frames and --obj: the OBJ twisted through hpt_scene_set_skin once and hpt_scene_skin per frame: two
//                     bones, bone 0 at identity and bone 1 --spin-device's turn of f * DEG; a corner of the OBJ follows bone 1 by
//                     its height in the mesh, so the foot stays put and the top turns; not together with --spin, --spin-device
//   --rebuild-above R with --frames and --spin, --spin-device or --twist-device: measure the tree's cost (hpt_scene_tree_cost) after
//                     each frame's update and rebuild the tree in place (hpt_scene_rebuild) when its sah exceeds R times the
//                     cost of the last built tree; one "[Rebuild]" line per rebuild.  R must be above 1.  Same image.
//   --rebuild-device  with --frames and --spin, --spin-device, --twist-device or --morph-device: the rebuilds of --rebuild-above are
//                     built on the device (hpt_scene_rebuild_device); without --rebuild-above the tree is rebuilt on the device
//                     before every frame that follows an update.  Same image.
//   --rebuild-depth D with --rebuild-device: its builds are bounded ones (hpt_scene_rebuild_device_bounded) of at most D levels;
//                     D is 0 (the traversal's 30) or 1 .. 30, and 19 or less never falls back to the host builder.  Same image.
//   --morph-device AMP with --frames and --obj: the OBJ morphed through hpt_scene_set_morphs once and hpt_scene_morph per frame: two
//                     targets on the OBJ's corners, an outward push and a lift that both grow with the corner's height in the mesh,
//                     under weights that swing with the frame; combines with --spin-device or --twist-device (morph, then the
//                     deformer); not together with --spin
//   --reproject       with --frames: keep the accumulated frames across camera moves (hpt_history): frame 0 and every moved
//                     frame render --guide-spp guide samples, and each pixel carries its mean and sample count over from
//                     where its surface point was a frame ago; the frame's line ends in "kept <share> %".
//   --guided          with --frames: present the variance-guided filter of the accumulated mean (hpt_denoiser_run_guided)
//                     instead of the mean: guides with albedo on frame 0 and every moved frame (--guide-spp >= 1), the
//                     variance from the accumulator's moments or, in the first frames and under --reproject, from the
//                     spatial estimate of the new frame divided by the history length.
//   --temporal-variance   with --frames --reproject --guided: the history also carries each pixel's second moment
//                     (HPT_HISTORY_MOMENTS), and where a pixel's history is at least four frames long its own variance
//                     over time (hpt_history_variance) replaces the spatial estimate.
// --mode pt, bdpt, ppm and sppm are built; bdpt renders the reference's CPU estimator (run_cpu_bdpt) on the GPU, ppm the
// reference's photon mapping (ppm_cu.cu) with a gather in a fixed order: --spp passes of --spl photons per light,
// averaged, on one device; sppm the same passes into one progressive state whose radius shrinks per pixel.
#include "scene_model.hpp"
#include "frame_loop.hpp"
#include "../../../include/hpt.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#define LIGHT_DEPTH 4
#define EYE_DEPTH 4

namespace hpt_host { extern hpt_params g_run_params; extern bool g_seed_from_clock; extern int g_devices; extern float g_ppm_radius; extern float g_sppm_alpha; }

int main(int argc, char **argv){
    int spp = 8, spl = 8;
    std::string mode = "pt", output_file = "output.png", input_file = "../../input.txt", device = "gpu", obj_file;
    int width = 0, height = 0, max_depth = EYE_DEPTH;
    long long seed = -1;
    bool denoise = false;
    int guide_spp = 4;
    hpt_denoise_params filter = { 0, 0.0f, 0.0f, 0.0f, 0 };
    int frames = 0, frame_spp = 0;
    double until_rms = -1.0;
    std::string rms_log;
    double orbit_deg = 0.0, spin_deg = 0.0;
    bool spin = false, spin_device = false, twist_device = false, morph_device = false;
    double morph_amp = 0.0;
    bool orbit = false, reproject = false, guided = false, temporal_variance = false;
    bool rebuild = false; double rebuild_above = 0.0;
    bool rebuild_device = false; int rebuild_depth = -1;
    for(int i = 1; i < argc; ++i){
        std::string arg = argv[i];
        if(arg == "--spp" && i + 1 < argc) spp = std::stoi(argv[++i]);
        else if(arg == "--spl" && i + 1 < argc) spl = std::stoi(argv[++i]);
        else if(arg == "--mode" && i + 1 < argc) mode = argv[++i];
        else if(arg == "--device" && i + 1 < argc) device = argv[++i];
        else if(arg == "--output" && i + 1 < argc) output_file = argv[++i];
        else if(arg == "--input" && i + 1 < argc) input_file = argv[++i];
        else if(arg == "--width" && i + 1 < argc) width = std::stoi(argv[++i]);
        else if(arg == "--height" && i + 1 < argc) height = std::stoi(argv[++i]);
        else if(arg == "--seed" && i + 1 < argc) seed = std::stoll(argv[++i]);
        else if(arg == "--max-depth" && i + 1 < argc) max_depth = std::stoi(argv[++i]);
        else if(arg == "--obj" && i + 1 < argc) obj_file = argv[++i];
        else if(arg == "--rr") hpt_host::g_run_params.flags |= HPT_FLAG_RUSSIAN_ROULETTE;
        else if(arg == "--gpus" && i + 1 < argc) hpt_host::g_devices = std::max(1, std::stoi(argv[++i]));
        else if(arg == "--radius" && i + 1 < argc) hpt_host::g_ppm_radius = std::stof(argv[++i]);
        else if(arg == "--alpha" && i + 1 < argc) hpt_host::g_sppm_alpha = std::stof(argv[++i]);
        else if(arg == "--denoise") denoise = true;
        else if(arg == "--guide-spp" && i + 1 < argc) guide_spp = std::stoi(argv[++i]);
        else if(arg == "--denoise-iterations" && i + 1 < argc) filter.iterations = std::stoi(argv[++i]);
        else if(arg == "--sigma-color" && i + 1 < argc) filter.sigma_color = std::stof(argv[++i]);
        else if(arg == "--sigma-normal" && i + 1 < argc) filter.sigma_normal = std::stof(argv[++i]);
        else if(arg == "--sigma-position" && i + 1 < argc) filter.sigma_position = std::stof(argv[++i]);
        else if(arg == "--frames" && i + 1 < argc) frames = std::stoi(argv[++i]);
        else if(arg == "--frame-spp" && i + 1 < argc) frame_spp = std::stoi(argv[++i]);
        else if(arg == "--until-rms" && i + 1 < argc) until_rms = std::stod(argv[++i]);
        else if(arg == "--rms-log" && i + 1 < argc) rms_log = argv[++i];
        else if(arg == "--orbit" && i + 1 < argc){ orbit_deg = std::stod(argv[++i]); orbit = true; }
        else if(arg == "--spin" && i + 1 < argc){ spin_deg = std::stod(argv[++i]); spin = true; }
        else if(arg == "--spin-device" && i + 1 < argc){ spin_deg = std::stod(argv[++i]); spin_device = true; }
        else if(arg == "--twist-device" && i + 1 < argc){ spin_deg = std::stod(argv[++i]); twist_device = true; }
        else if(arg == "--rebuild-above" && i + 1 < argc){ rebuild_above = std::stod(argv[++i]); rebuild = true; }
        else if(arg == "--rebuild-device") rebuild_device = true;
        else if(arg == "--rebuild-depth" && i + 1 < argc){
            char *end = nullptr; const long d = std::strtol(argv[++i], &end, 10);
            if(!end || *end || end == argv[i] || d < 0 || d > 30){ std::cerr << "[Error] --rebuild-depth needs 0 or a depth of 1 to 30.\n"; return -1; }
            rebuild_depth = (int) d;
        }
        else if(arg == "--morph-device" && i + 1 < argc){ morph_amp = std::stod(argv[++i]); morph_device = true; }
        else if(arg == "--reproject") reproject = true;
        else if(arg == "--guided") guided = true;
        else if(arg == "--temporal-variance") temporal_variance = true;
        else if(arg == "--help" || arg == "-h"){
            std::cout << "Usage: pt_cli [options]\n"
                      << "Options:\n"
                      << "  --spp <int>       Samples per pixel (default: 8)\n"
                      << "  --spl <int>       Samples per light (default: 8)\n"
                      << "  --mode <string>   Render mode: pt, bdpt, ppm, sppm (default: pt)\n"
                      << "  --device <string> Compute device: gpu (default: gpu)\n"
                      << "  --output <string> Output image path (.png or .pfm)\n"
                      << "  --input <string>  Input scene file\n"
                      << "  --width/--height <int>  override the scene's R line\n"
                      << "  --seed <int>      reproducible random streams (default: clock)\n"
                      << "  --max-depth <int> eye depth (default: 4)\n"
                      << "  --obj <file>      append the faces of a Wavefront OBJ\n"
                      << "  --rr              unbiased Russian roulette (pt mode; not in the reference, off by default)\n"
                      << "  --gpus <int>      devices of this node to render on (image tiles, RCCL gather; default: 1; pt and bdpt)\n"
                      << "  --radius <float>  photon search radius of ppm mode, initial radius of sppm mode (default: 0.05)\n"
                      << "  --alpha <float>   radius reduction of sppm mode, in (0, 1] (default: 0.7); --spp is its number of passes\n"
                      << "  --denoise         denoise the frame before saving it (every mode; with --gpus on device 0)\n"
                      << "  --guide-spp <int> guide samples per pixel of --denoise (default: 4)\n"
                      << "  --denoise-iterations <int>  filter levels, 1..8 (default: 5)\n"
                      << "  --sigma-color/--sigma-normal/--sigma-position <float>  edge-stopping widths (defaults: 1.0, 0.5, 0.05; < 0: off)\n"
                      << "  --frames <int>    progressive: frames to accumulate and present on the device (pt, bdpt, ppm; one device)\n"
                      << "  --frame-spp <int> samples (ppm: passes) per frame (default: --spp)\n"
                      << "  --until-rms <float>  stop after a frame >= 2 whose RMS against the previous frame is <= this\n"
                      << "  --rms-log <file>  one line \"<frame> <rms>\" per frame\n"
                      << "  --orbit <deg>     with --frames: frame f renders from the eye rotated by f * deg degrees about the look-at point\n"
                      << "                    around the up vector; the accumulation restarts on every moved frame\n"
                      << "  --spin <deg>      with --frames and --obj: before frame f the OBJ's triangles are turned by f * deg degrees about the\n"
                      << "                    vertical axis through their centroid (hpt_scene_update_triangles); with --reproject the history\n"
                      << "                    follows them through the motion guide, without it the accumulation restarts after every update\n"
                      << "  --spin-device <deg>  --spin with the OBJ as one rigid part posed on the device (hpt_scene_set_parts once,\n"
                      << "                    hpt_scene_pose per frame): the same turn as a 3 x 4 matrix rounded to float, twelve floats per\n"
                      << "                    frame and no record copied.  The pose multiplies in float where --spin turns in double and\n"
                      << "                    rounds once, so the images differ from --spin's in the last bits.  Not together with --spin\n"
                      << "  --twist-device <deg>  with --frames and --obj: the OBJ twisted by a two-bone skin on the device (hpt_scene_set_skin\n"
                      << "                    once, hpt_scene_skin per frame): bone 1 is --spin-device's turn of f * deg and a corner follows it by\n"
                      << "                    its height in the mesh, so the foot stays put and the top turns.  Not together with --spin or\n"
                      << "                    --spin-device\n"
                      << "  --rebuild-above <R>  with --frames and --spin, --spin-device or --twist-device: rebuild the tree in place when its\n"
                      << "                    cost (sah of hpt_scene_tree_cost) exceeds R times the last built tree's; R > 1\n"
                      << "  --rebuild-device  the rebuilds of --rebuild-above are built on the device (hpt_scene_rebuild_device); without\n"
                      << "                    --rebuild-above the tree is rebuilt on the device before every frame that follows an update\n"
                      << "  --rebuild-depth <D>  with --rebuild-device: its builds are bounded to D levels (hpt_scene_rebuild_device_bounded);\n"
                      << "                    D is 0 (the traversal's 30) or 1 to 30; 19 or less never falls back to the host builder\n"
                      << "  --morph-device <amp>  with --frames and --obj: the OBJ morphed by two targets on the device (hpt_scene_set_morphs once,\n"
                      << "                    hpt_scene_morph per frame): target 0 pushes a corner away from the vertical axis through the centroid,\n"
                      << "                    target 1 lifts it, both by the corner's height in the mesh times a quarter of the OBJ's radius; the\n"
                      << "                    weights at frame f are amp * (1 - cos(2 pi f / 32)) / 2 and amp * sin(2 pi f / 32).  Combines with\n"
                      << "                    --spin-device or --twist-device (morph, then the deformer).  Not together with --spin\n"
                      << "  --reproject       with --frames: keep the accumulation across camera moves by reprojecting it through\n"
                      << "                    --guide-spp guide samples per moved frame; prints the share of pixels kept\n"
                      << "  --guided          with --frames: present the mean filtered under its per-pixel variance (needs --guide-spp >= 1)\n"
                      << "  --temporal-variance  with --frames --reproject --guided: carry second moments through the history and use each\n"
                      << "                    pixel's variance over time where its history is at least four frames long\n";
            return 0;
        }
    }
    std::cout << "====================================\n";
    std::cout << " Device : " << device << "\n";
    std::cout << " Mode   : " << mode << "\n";
    std::cout << " SPP    : " << spp << "\n";
    std::cout << " SPL    : " << spl << " (used in BDPT/PPM)\n";
    std::cout << " Input  : " << input_file << "\n";
    std::cout << " Output : " << output_file << "\n";
    std::cout << "====================================\n";
    if(mode != "pt" && mode != "bdpt" && mode != "ppm" && mode != "sppm"){ std::cerr << "[Error] unknown mode " << mode << " (pt, bdpt, ppm, sppm).\n"; return -1; }
    const bool progressive = frames != 0 || frame_spp != 0 || until_rms >= 0.0 || !rms_log.empty();
    if(temporal_variance && (frames < 1 || !reproject || !guided)){
        std::cerr << "[Error] --temporal-variance needs --frames N (N >= 1), --reproject and --guided.\n"; return -1;
    }
    if((orbit || reproject) && frames < 1){ std::cerr << "[Error] --orbit and --reproject need --frames N (N >= 1).\n"; return -1; }
    if(rebuild && !(rebuild_above > 1.0 && std::isfinite(rebuild_above))){ std::cerr << "[Error] --rebuild-above needs a finite ratio above 1.\n"; return -1; }
    if(rebuild && (frames < 1 || !(spin || spin_device || twist_device || morph_device))){
        std::cerr << "[Error] --rebuild-above needs --frames and one of --spin, --spin-device, --twist-device, --morph-device.\n"; return -1;
    }
    if(morph_device && spin){ std::cerr << "[Error] --morph-device and --spin exclude each other.\n"; return -1; }
    if(morph_device && (frames < 1 || obj_file.empty())){ std::cerr << "[Error] --morph-device needs --frames and --obj.\n"; return -1; }
    if(morph_device && !std::isfinite(morph_amp)){ std::cerr << "[Error] --morph-device needs a finite amplitude.\n"; return -1; }
    if(spin && spin_device){ std::cerr << "[Error] --spin and --spin-device exclude each other.\n"; return -1; }
    if(twist_device && (spin || spin_device)){ std::cerr << "[Error] --twist-device and " << (spin ? "--spin" : "--spin-device") << " exclude each other.\n"; return -1; }
    if(twist_device && (frames < 1 || obj_file.empty())){ std::cerr << "[Error] --twist-device needs --frames and --obj.\n"; return -1; }
    if(twist_device && !std::isfinite(spin_deg)){ std::cerr << "[Error] --twist-device needs a finite angle.\n"; return -1; }
    if(spin_device && (frames < 1 || obj_file.empty())){ std::cerr << "[Error] --spin-device needs --frames and --obj.\n"; return -1; }
    if(spin_device && !std::isfinite(spin_deg)){ std::cerr << "[Error] --spin-device needs a finite angle.\n"; return -1; }
    if(spin && (frames < 1 || obj_file.empty())){ std::cerr << "[Error] --spin needs --frames and --obj.\n"; return -1; }
    if(spin && !std::isfinite(spin_deg)){ std::cerr << "[Error] --spin needs a finite angle.\n"; return -1; }
    if(guided && frames < 1){ std::cerr << "[Error] --guided needs --frames N (N >= 1).\n"; return -1; }
    if(guided && guide_spp < 1){ std::cerr << "[Error] --frames --guided needs --guide-spp of at least 1.\n"; return -1; }
    if(orbit && !std::isfinite(orbit_deg)){ std::cerr << "[Error] --orbit needs a finite angle.\n"; return -1; }
    if(progressive){
        if(frames < 1){ std::cerr << "[Error] --frame-spp, --until-rms and --rms-log need --frames N (N >= 1).\n"; return -1; }
        if(mode == "sppm"){ std::cerr << "[Error] --frames does not apply to --mode sppm: it keeps its own progressive state (use --spp for its passes).\n"; return -1; }
        if(hpt_host::g_devices > 1){ std::cerr << "[Error] --frames renders on one device: it cannot be combined with --gpus above 1.\n"; return -1; }
        if(frame_spp == 0) frame_spp = spp;
        if(frame_spp < 1){ std::cerr << "[Error] --frame-spp must be at least 1.\n"; return -1; }
    }

    hpt_host::SceneFile scene;
    if(!hpt_host::parse_scene_file(input_file, scene)){
        std::cerr << "[Error] Cannot open input file: " << input_file << "\n";
        return -1;
    }
    int first_obj_id = 0;                  // the OBJ's faces are numbered from here on
    for(const hpt_host::SceneItem &it : scene.items) first_obj_id = std::max(first_obj_id, it.obj_id + 1);
    if(!obj_file.empty()){
        hpt_host::Material grey; grey.base_color = {0.7f, 0.7f, 0.7f}; grey.roughness = 1.0f;
        std::string err;
        int n = hpt_host::append_obj(obj_file, grey, 2, scene, &err);
        if(n < 0){ std::cerr << "[Error] " << err << "\n"; return -1; }
        std::cout << "OBJ triangles: " << n << std::endl;
    }
    std::cout << "[Parse] " << scene.parse_ms << " ms\n";
    std::cout << "Ball:" << std::endl << scene.ball_cnt << std::endl;
    std::cout << "Triangle:" << std::endl << scene.tri_cnt << std::endl;
    std::cout << "Light:" << std::endl << scene.lights.size() << std::endl;

    const int W = width > 0 ? width : scene.resolution.first;
    const int H = height > 0 ? height : scene.resolution.second;
    if(rebuild_device && (frames < 1 || !(spin || spin_device || twist_device || morph_device))){
        std::cerr << "[Error] --rebuild-device needs --frames and one of --spin, --spin-device, --twist-device, --morph-device.\n"; return -1;
    }
    if(rebuild_depth >= 0 && !rebuild_device){ std::cerr << "[Error] --rebuild-depth needs --rebuild-device.\n"; return -1; }
    float F = 50;
    CudaCamera cam = hpt_host::make_cuda_camera(scene.camera, F, W, H);
    std::vector<float3> frame_results((size_t) W * H);

    std::cout << "[Init] Transferring Data to the GPU...\n";
    if(mode == "bdpt") move_data_to_cuda_bdpt(scene.groups(), scene.lights, spl);
    else if(mode == "ppm" || mode == "sppm") move_data_to_cuda_ppm(scene.groups(), scene.lights, spl);
    else move_data_to_cuda_pt(scene.groups(), scene.lights, spl);
    if(seed >= 0){ hpt_host::g_seed_from_clock = false; hpt_host::g_run_params.seed = (uint64_t) seed; }

    std::cout << "[Render] Starting Render...\n";
    auto start_time = std::chrono::steady_clock::now();
    std::vector<unsigned char> presented;
    if(progressive){
        hpt_host::FrameMotion motion;
        motion.reproject = reproject; motion.guide_spp = guide_spp; motion.guided = guided; motion.temporal_variance = temporal_variance;
        motion.rebuild_above = rebuild ? rebuild_above : 0.0;
        motion.rebuild_device = rebuild_device;
        motion.rebuild_depth = rebuild_depth;
        if(orbit) motion.camera_at = [&](int f, void *camera84){
            // Rodrigues' rotation of eye - look_at about the unit up vector, in double
            const hpt_host::Camera &c = scene.camera;
            const double e[3] = { c.eye.x, c.eye.y, c.eye.z }, l[3] = { c.look_at.x, c.look_at.y, c.look_at.z };
            double k[3] = { c.view_up.x, c.view_up.y, c.view_up.z };
            const double len = std::sqrt(k[0] * k[0] + k[1] * k[1] + k[2] * k[2]);
            for(double &x : k) x /= len;
            const double v[3] = { e[0] - l[0], e[1] - l[1], e[2] - l[2] };
            const double t = (double) f * orbit_deg * 3.14159265358979323846 / 180.0, cs = std::cos(t), sn = std::sin(t);
            const double kxv[3] = { k[1] * v[2] - k[2] * v[1], k[2] * v[0] - k[0] * v[2], k[0] * v[1] - k[1] * v[0] };
            const double kv = (k[0] * v[0] + k[1] * v[1] + k[2] * v[2]) * (1.0 - cs);
            hpt_host::Camera moved = c;
            moved.eye.x = (float) (l[0] + (v[0] * cs + kxv[0] * sn + k[0] * kv));
            moved.eye.y = (float) (l[1] + (v[1] * cs + kxv[1] * sn + k[1] * kv));
            moved.eye.z = (float) (l[2] + (v[2] * cs + kxv[2] * sn + k[2] * kv));
            const CudaCamera cc = hpt_host::make_cuda_camera(moved, F, W, H);
            memcpy(camera84, &cc, sizeof cc);
        };
        if(spin) motion.triangles_at = [&](int f, void *triangles, int count){
            // frame f: the ORIGINAL vertices of the OBJ's triangles turned by f * deg about the y axis through their centroid,
            // in double, so that rounding does not accumulate over the frames
            CudaTriangle *tr = (CudaTriangle *) triangles;
            double c[3] = { 0.0, 0.0, 0.0 }, n = 0.0;
            for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                for(const float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }){ c[0] += v->x; c[1] += v->y; c[2] += v->z; n += 1.0; }
            }
            if(n == 0.0) return;
            for(double &x : c) x /= n;
            const double t = (double) f * spin_deg * 3.14159265358979323846 / 180.0, cs = std::cos(t), sn = std::sin(t);
            for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                for(float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }){
                    const double x = v->x - c[0], z = v->z - c[2];
                    v->x = (float) (c[0] + x * cs + z * sn);
                    v->z = (float) (c[2] - x * sn + z * cs);
                }
            }
        };
        double spin_centre[3] = { 0.0, 0.0, 0.0 };
        if(spin_device){
            // part 0: everything that is not the OBJ, left at identity; part 1: the OBJ.  The centroid is --spin's, in double
            motion.parts_of = [&](const void *triangles, int count, std::vector<int32_t> &tri_part){
                const CudaTriangle *tr = (const CudaTriangle *) triangles;
                tri_part.assign((size_t) count, 0);
                double c[3] = { 0.0, 0.0, 0.0 }, n = 0.0;
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    tri_part[(size_t) i] = 1;
                    for(const float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }){ c[0] += v->x; c[1] += v->y; c[2] += v->z; n += 1.0; }
                }
                if(n != 0.0) for(int a = 0; a < 3; ++a) spin_centre[a] = c[a] / n;
                return 2;
            };
            // frame f: --spin's turn, x' = c + R (x - c) = R x + (c - R c), as three rows (a, b, c, t) rounded to float
            motion.pose_at = [&](int f, float *xforms, int num_parts){
                static const float identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
                for(int k = 0; k < num_parts; ++k) memcpy(xforms + 12 * k, identity, sizeof identity);
                if(num_parts < 2) return;
                const double *c = spin_centre;
                const double t = (double) f * spin_deg * 3.14159265358979323846 / 180.0, cs = std::cos(t), sn = std::sin(t);
                float *r = xforms + 12;
                r[0] = (float) cs; r[2] = (float) sn; r[3] = (float) (c[0] - (c[0] * cs + c[2] * sn));
                r[8] = (float) -sn; r[10] = (float) cs; r[11] = (float) (c[2] - (-c[0] * sn + c[2] * cs));
            };
        }
        if(twist_device){
            // two bones: bone 0 stays at identity, bone 1 is --spin-device's turn.  A corner of the OBJ at height y follows bone 1
            // with t = clamp((y - ymin) / (ymax - ymin), 0, 1) and bone 0 with 1 - t, in float; every other corner has four zero
            // weights and keeps its bits
            motion.skin_of = [&](const void *triangles, int count, std::vector<int32_t> &corner_bone, std::vector<float> &corner_weight){
                const CudaTriangle *tr = (const CudaTriangle *) triangles;
                corner_bone.assign((size_t) count * 12, 0);
                corner_weight.assign((size_t) count * 12, 0.0f);
                double c[3] = { 0.0, 0.0, 0.0 }, n = 0.0;
                float ymin = INFINITY, ymax = -INFINITY;
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    for(const float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }){
                        c[0] += v->x; c[1] += v->y; c[2] += v->z; n += 1.0;
                        ymin = std::min(ymin, v->y); ymax = std::max(ymax, v->y);
                    }
                }
                if(n != 0.0) for(int a = 0; a < 3; ++a) spin_centre[a] = c[a] / n;
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    const float3 *vs[3] = { &tr[i].v0, &tr[i].v1, &tr[i].v2 };
                    for(int k = 0; k < 3; ++k){
                        float t = ymax > ymin ? (vs[k]->y - ymin) / (ymax - ymin) : 0.0f;
                        t = t > 0.0f ? (t < 1.0f ? t : 1.0f) : 0.0f;                  // (a NaN height: 0, the foot)
                        const size_t at = ((size_t) i * 3 + (size_t) k) * 4;
                        corner_bone[at + 1] = 1;
                        corner_weight[at] = 1.0f - t; corner_weight[at + 1] = t;
                    }
                }
                return 2;
            };
            motion.skin_at = [&](int f, float *xforms, int num_bones){
                static const float identity[12] = { 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0 };
                for(int k = 0; k < num_bones; ++k) memcpy(xforms + 12 * k, identity, sizeof identity);
                if(num_bones < 2) return;
                const double *c = spin_centre;
                const double t = (double) f * spin_deg * 3.14159265358979323846 / 180.0, cs = std::cos(t), sn = std::sin(t);
                float *r = xforms + 12;
                r[0] = (float) cs; r[2] = (float) sn; r[3] = (float) (c[0] - (c[0] * cs + c[2] * sn));
                r[8] = (float) -sn; r[10] = (float) cs; r[11] = (float) (c[2] - (-c[0] * sn + c[2] * cs));
            };
        }
        if(morph_device){
            // two targets over the OBJ's corners, in corner order.  h = clamp((y - ymin) / (ymax - ymin), 0, 1) is a corner's height
            // in the mesh and r the largest distance of a corner from the vertical axis through the centroid, in double; target 0
            // moves the corner away from that axis by h * r / 4, target 1 lifts it by the same amount; rounded to float once
            motion.morphs_of = [&](const void *triangles, int count, std::vector<int32_t> &target_begin, std::vector<int32_t> &entry_corner,
                                   std::vector<float> &entry_delta){
                const CudaTriangle *tr = (const CudaTriangle *) triangles;
                double c[3] = { 0.0, 0.0, 0.0 }, n = 0.0, ymin = INFINITY, ymax = -INFINITY, radius = 0.0;
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    for(const float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }){
                        c[0] += v->x; c[1] += v->y; c[2] += v->z; n += 1.0;
                        ymin = std::min(ymin, (double) v->y); ymax = std::max(ymax, (double) v->y);
                    }
                }
                if(n != 0.0) for(double &x : c) x /= n;
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    for(const float3 *v : { &tr[i].v0, &tr[i].v1, &tr[i].v2 }) radius = std::max(radius, std::hypot(v->x - c[0], v->z - c[2]));
                }
                std::vector<float> lift;
                entry_corner.clear(); entry_delta.clear();
                for(int i = 0; i < count; ++i) if(tr[i].id >= first_obj_id){
                    const float3 *vs[3] = { &tr[i].v0, &tr[i].v1, &tr[i].v2 };
                    for(int k = 0; k < 3; ++k){
                        double h = ymax > ymin ? (vs[k]->y - ymin) / (ymax - ymin) : 0.0;
                        h = h > 0.0 ? (h < 1.0 ? h : 1.0) : 0.0;                      // (a NaN height: 0, the foot)
                        const double x = vs[k]->x - c[0], z = vs[k]->z - c[2], d = std::hypot(x, z), by = h * radius / 4.0;
                        entry_corner.push_back(i * 3 + k);
                        entry_delta.push_back(d > 0.0 ? (float) (x / d * by) : 0.0f);
                        entry_delta.push_back(0.0f);
                        entry_delta.push_back(d > 0.0 ? (float) (z / d * by) : 0.0f);
                        lift.push_back((float) by);
                    }
                }
                const size_t per_target = entry_corner.size();
                entry_corner.insert(entry_corner.end(), entry_corner.begin(), entry_corner.begin() + (long) per_target);
                for(float by : lift){ entry_delta.push_back(0.0f); entry_delta.push_back(by); entry_delta.push_back(0.0f); }
                target_begin = { 0, (int32_t) per_target, (int32_t) (2 * per_target) };
                return 2;
            };
            motion.morph_at = [&](int f, float *weights, int num_targets){
                const double t = 2.0 * 3.14159265358979323846 * (double) f / 32.0;
                if(num_targets > 0) weights[0] = (float) (morph_amp * (1.0 - std::cos(t)) / 2.0);
                if(num_targets > 1) weights[1] = (float) (morph_amp * std::sin(t));
            };
        }
        const int n = hpt_host::run_frame_loop(mode, &cam, &frame_results[0].x, presented, LIGHT_DEPTH, max_depth, W, H, frames, frame_spp,
                                               spl, hpt_host::g_ppm_radius, until_rms, rms_log,
                                               orbit || reproject || guided || spin || spin_device || twist_device || morph_device ? &motion : nullptr);
        if(n < 0) return -1;
        std::cout << "[Render] " << n << " frames of " << frame_spp << " spp";
    }
    else if(mode == "bdpt") run_cuda_bdpt(cam, frame_results.data(), LIGHT_DEPTH, max_depth, W, H, spp, spl);
    else if(mode == "ppm") run_cuda_ppm(cam, frame_results.data(), LIGHT_DEPTH, max_depth, W, H, spp);
    else if(mode == "sppm") run_cuda_sppm(cam, frame_results.data(), LIGHT_DEPTH, max_depth, W, H, spp);
    else run_cuda_pt(cam, frame_results.data(), LIGHT_DEPTH, max_depth, W, H, spp);
    std::cout << "\n";
    auto diff = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - start_time);
    std::cout << "[Render] Finished in " << diff.count() << " ms.\n";

    if(denoise){
        auto t0 = std::chrono::steady_clock::now();
        if(!denoise_frame(mode, cam, frame_results.data(), W, H, guide_spp, filter)) return -1;
        auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::steady_clock::now() - t0);
        std::cout << "[Denoise] " << guide_spp << " guide spp, finished in " << ms.count() << " ms.\n";
    }

    std::cout << "[Save] Writing to " << output_file << "...\n";
    std::string err;
    const bool png = !(output_file.size() > 4 && output_file.compare(output_file.size() - 4, 4, ".pfm") == 0);
    // a progressive run's PNG holds the last presented bytes (a denoised frame is tone-mapped afresh)
    const bool ok = progressive && !denoise && png ? hpt_host::write_png_rgb8(output_file, presented.data(), W, H, &err)
                                                   : hpt_host::write_image(output_file, frame_results.data(), W, H, &err);
    if(ok) std::cout << "[Success] Image saved!\n";
    else std::cerr << "[Error] Failed to save image.\n";
    return 0;
}
