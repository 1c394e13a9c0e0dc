// snesimage_amd/csrc/cli.cpp — headless driver over the C ABI, keeping the reference's command line
// (src/config.rs:3-31: source_filename target_filename [-c N] [-s N] [-d] [--perceptual-palettes]
// [--nes]) and its JSON output (src/lib.rs:579-625, 1002).  The reference drives the optimizer from
// an SDL2 window (src/lib.rs:855-1038, out of scope); here the three phases advance on their own:
// TileAssignment (initialize_tiles) -> Clustering (recalculate_palettes) -> Optimization for
// --calls optimizer calls in the reference's slot order (src/lib.rs:881-933) -> write the JSON.
// Extra flags exist only because the reference is interactive and unseeded: --seed, --calls,
// --candidates, --device, --tile-palettes FILE (1024 bytes, replaces the mouse clicks of
// src/lib.rs:1005-1017), --resume FILE.json (start from a previous output instead of the k-means initialisers: the
// reference's TODO.md:38-39), --preview FILE.png (source | result side by side, the picture the SDL window of
// src/lib.rs:937-960 shows).  The source image is a PNG (png_io.hpp restates `image::open(..).into_rgba8()`,
// src/lib.rs:836, for that format), a raw RGBA8 file of 256*H*4 bytes, or `synth:SEED`.
// --backdrop gives every tile one more colour, the SNES backdrop colour shared by all tiles (include/snesimage_hip.h:
// SNES_BACKDROP), optimized like any entry; --backdrop-fixed R,G,B (5-bit) keeps it at the given colour.
// --set-backdrop / --set-backdrop-fixed R,G,B do the same for a --share set (snesimage_shared_create_backdrop): one backdrop colour
// for all frames, decided on the set's error; with them --resume restarts every frame from its own earlier JSON.
// --share SOURCE=TARGET (repeatable) optimizes one palette for the main image and every such image together (a set,
// include/snesimage_hip.h): the frames of an animation share one CGRAM on the console.
// --ordered-dither N [--dither-amplitude A] adds the N x N Bayer pattern of amplitude A to the picture before the nearest-colour
// choice (include/snesimage_hip.h: snesimage_set_ordered_dither): the alternative to -d that keeps animation frames steady.
// The JSON does not record it: a --resume run names the option again.
// --palette-blocks WxH (include/snesimage_hip.h: "Palette blocks") gives one subpalette per block of W x H tiles instead of per
// tile; it is set before the initialisers, --reassign-tiles then moves whole blocks and --tile-moves runs block sweeps.  The
// JSON stays per tile and does not record it either.
// --tile-dither K [--dither-levels L] lets every tile choose its own strength of that pattern (include/snesimage_hip.h:
// snesimage_level_sweep): a ladder of L amplitudes from none to A, every tile starting on A; every K sweeps of the palette and
// once behind the last call each tile is tried on every other level and kept where the error itself falls.
// --tile-levels-out FILE / --tile-levels-in FILE carry the ladder and the tiles' levels from run to run (for --resume).
// --set-tile-dither K (with --share and --ordered-dither) does the same for a set (include/snesimage_hip.h:
// snesimage_shared_level_sweep): --set-levels tied (the default) keeps one level per tile position for all frames, decided on the
// set's error, so a static tile's pattern does not switch on and off from frame to frame; --set-levels frame lets every frame
// choose for itself.  --set-tile-levels-out FILE / --set-tile-levels-in FILE carry the ladder and every frame's levels.
// --max-tiles N merges tiles after the last optimizer call until at most N distinct characters are left (the VRAM budget;
// include/snesimage_hip.h: snesimage_reduce_characters), --merge-shortlist K sets how many merges each step scores, and
// --tilemap FILE writes the characters and the tilemap (snesimage_as_tilemap_json), with or without --max-tiles.
// --refit-tiles N runs up to N refit sweeps behind that (snesimage_refit_characters): every shared character is refitted to all
// the tiles that use it, and the refit is kept where the error falls.
// --max-set-tiles N (with --share) is the budget of the whole set: the frames share one VRAM character area, so their characters
// are counted together and a tile may take its indices from a tile of another frame (snesimage_shared_reduce_characters);
// --set-tilemap FILE writes the set's characters and one tilemap per frame (snesimage_shared_as_tilemap_json).
// --export-cgram / --export-chr / --export-map FILE write the result as the console loads it (snesimage_export_native), the
// --set-export- trio that of a --share set (snesimage_shared_export_native); --export-bpp, --export-char-base,
// --export-palette-base and --export-priority lay it out.  The bytes are rendered back (snesimage_render_native) and compared
// with as_rgba() before a file is written.
// --import-cgram / --import-chr / --import-map FILE (all three) start the run from native data instead of the k-means initialisers
// (snesimage_import_native): the export's own files, or bytes from a ROM or a tile editor; --import-bpp, --import-char-base and
// --import-palette-base describe them, apart from the --export- options, so a run can read one layout and write another.  The
// --set-import- trio does the same for a --share set (snesimage_shared_import_native).  With --calls 0 the imported state is what is
// written, after --max-tiles / --refit-tiles (--max-set-tiles / --refit-set-tiles) if they are given.
// --refit-set-tiles N (with --share) runs up to N refit sweeps over the whole set behind that (snesimage_shared_refit_characters):
// every character shared by tiles of whichever frames is refitted to all of them, and kept where the set's error falls.
// --guided G runs, behind every G sweeps of the palette, one guided sweep (include/snesimage_hip.h: snesimage_guided_run_slots, --window calls per launch set): on every
// slot the --guided-shortlist K colours an integer proxy ranks best among all 32,768 are scored, and the error decides.
// --guided-proxy / --set-guided-proxy redmean|cielab choose the proxy's distance (snesimage_set_guided_proxy; DESIGN 5f'').
// --set-guided G (with --share) does the same for a set (snesimage_shared_guided_run_slots): the proxy runs over the tiles of all
// frames, every frame scores the --set-guided-shortlist K colours, and the set's error decides.
// The host language the north star asks for is Rust; no Rust toolchain exists in this image, so the
// driver is C++ over the same extern "C" surface a Rust crate would bind.
#include "../../include/snesimage_hip.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <algorithm>
#include <string>
#include <vector>

#include "png_io.hpp"

namespace {

void log_info(const std::string &msg) { // src/util.rs:9-22: [time][level][target] message
    char ts[64];
    time_t now = time(nullptr);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&now));
    printf("[%s][INFO][snesimage] %s\n", ts, msg.c_str());
    fflush(stdout);
}
[[noreturn]] void die(const std::string &msg) { // src/main.rs:16-19
    char ts[64];
    time_t now = time(nullptr);
    strftime(ts, sizeof ts, "%Y-%m-%d %H:%M:%S", localtime(&now));
    printf("[%s][ERROR][snesimage] Error running application: %s\n", ts, msg.c_str());
    exit(1);
}
std::string fmt_f64(double v) { // Rust's `{}` for f64: shortest representation that round-trips
    char buf[64];
    for (int prec = 1; prec <= 17; prec++) {
        snprintf(buf, sizeof buf, "%.*g", prec, v);
        if (strtod(buf, nullptr) == v) break;
    }
    return buf;
}
void usage() {
    fprintf(stderr,
            "Usage: snesimage_cli [OPTIONS] <SOURCE_FILENAME> <TARGET_FILENAME>\n\n"
            "Arguments:\n  <SOURCE_FILENAME>  PNG image, raw RGBA8 file (256 x H x 4 bytes, H a multiple of 8 up to 256) or synth:SEED\n  <TARGET_FILENAME>  JSON output\n\n"
            "Options:\n  -c, --subpalette-count <N>  [default: 1]\n  -s, --subpalette-size <N>   [default: 7]\n"
            "  -d, --dither\n      --perceptual-palettes\n      --nes\n"
            "      --backdrop           one more colour for every tile: the backdrop colour (CGRAM word 0) shows where a tile has index 0;\n"
            "                           it is optimized like any entry and written to slot 0 of every palette row (needs -s <= 15,\n"
            "                           c*(s+1) <= 253; not with --share or --devices)\n"
            "      --backdrop-fixed <R,G,B>  the same with the backdrop colour given (5-bit channels) and never changed\n"
            "      --set-backdrop       with --share: the backdrop colour of the set, one CGRAM word 0 for all frames, optimized on the set's\n"
            "                           error; it starts as the mean of all frames' opaque pixels and is written to slot 0 of every palette\n"
            "                           row of every frame's JSON; --resume <F> then restarts the main frame from F and every --share frame\n"
            "                           from its own TARGET, the backdrop colour from slot 0 of F; not with --devices, --backdrop(-fixed),\n"
            "                           --max-set-tiles, --refit-set-tiles, --set-tilemap or the --set-tile-dither family\n"
            "      --set-backdrop-fixed <R,G,B>  the same with the backdrop colour given (5-bit channels) and never changed\n"
            "      --ordered-dither <N> ordered dithering with the N x N Bayer pattern (N = 2, 4, 8 or 16) instead of -d: a fixed pattern,\n"
            "                           so frames of an animation do not shimmer against each other; works with every other option\n"
            "                           but -d; the output does not record it: name it again with --resume\n"
            "      --dither-amplitude <A>  peak-to-peak strength of that pattern in 8-bit steps, 1..255 [default: 32, four BGR555 steps:\n"
            "                           a choice, not a measurement]\n"
            "      --tile-dither <K>    with --ordered-dither: every K sweeps of the palette and once behind the last call, try every tile on\n"
            "                           every other strength of the pattern (--dither-levels) and keep a change where the error itself\n"
            "                           falls; behind --tile-moves if both are given; not with -d, --share or --devices\n"
            "      --dither-levels <L>  strengths a tile chooses from, 2..8: level 0 is no dithering, level j the pattern at amplitude\n"
            "                           A*j/(L-1); needs A >= L-1; tiles start on the full amplitude [default: 4: a choice, not a\n"
            "                           measurement]\n"
            "      --tile-levels-out <F>  write the ladder and every tile's level as JSON ({\"n\", \"amplitudes\", \"levels\"})\n"
            "      --tile-levels-in <F>   start from the ladder and levels of such a file (with --resume: the main JSON does not record them);\n"
            "                           the ladder is the file's: a --dither-levels or --dither-amplitude that differs from it is refused\n"
            "      --set-tile-dither <K>  with --share and --ordered-dither: every K sweeps of the palette and once behind the last call, a\n"
            "                           level sweep of the set over all tiles (--dither-levels, --dither-amplitude: the same ladder; tiles\n"
            "                           start on the full amplitude); behind --tile-moves if both are given, in front of --max-set-tiles\n"
            "                           and --refit-set-tiles; not with -d or --devices\n"
            "      --set-levels <tied|frame>  tied: one level per tile position for all frames, decided on the set's error; frame: every\n"
            "                           frame chooses for itself [default: tied: a choice, made for steadiness from frame to frame, not a\n"
            "                           measurement]\n"
            "      --set-tile-levels-out <F>  write the ladder and every frame's levels as JSON ({\"n\", \"amplitudes\", \"tied\", \"frames\"}),\n"
            "                           frames in command-line order\n"
            "      --set-tile-levels-in <F>   start the set from the ladder and levels of such a file; the ladder is the file's: a\n"
            "                           --dither-levels or --dither-amplitude that differs from it is refused, as is a file with another\n"
            "                           frame or tile count, or one that says tied while its frames differ\n"
            "      --calls <N>          optimizer calls to run [default: 0]\n      --candidates <N>     random candidates per call [default: 64]\n"
            "      --window <N>         optimizer calls scored per launch set (0 = adaptive, 1 = call by call; same result) [default: 0]\n"
            "      --seed <N>           candidate RNG seed [default: 1]\n      --device <N>         HIP device [default: 0]\n"
            "      --devices <A,B,..>   shard every call's candidates over these devices (RCCL inside the library)\n"
            "      --tile-palettes <F>  1024-byte tile->subpalette override\n      --resume <F>         start from the palette and tile palettes of a previous JSON output\n"
            "      --preview <F>        write source | result as a PNG\n"
            "      --reassign-tiles <K> every K sweeps of the palette, move each tile to the subpalette that reproduces it best\n"
            "                           (off by default; not in the reference: its TODO.md lists it as missing)\n"
            "      --tile-moves <K>     every K sweeps of the palette, try every tile in every other subpalette and keep the moves that\n"
            "                           lower the error itself (dithering included); cannot be used with --reassign-tiles, which\n"
            "                           moves tiles by colour distance and undoes these moves, nor with --devices\n"
            "      --palette-blocks <WxH>  one subpalette per block of W x H tiles (W, H = 1, 2, 4 or 8; H divides the image's rows of\n"
            "                           tiles), such as 2x2 for the NES attribute table or an SNES background of 16 x 16 tiles, 4x4 or 8x8\n"
            "                           for sprites; set before the initialisers, which then cluster blocks; --reassign-tiles then moves\n"
            "                           whole blocks and --tile-moves tries whole blocks; not with --share, --devices or the --import-\n"
            "                           family; the output stays per tile and does not record it: name it again with --resume\n"
            "      --guided <G>         behind every G sweeps of the palette, one guided sweep: on every slot, all 32,768 colours are ranked by what\n"
            "                           the slot's pixels would cost in colour distance, and the --guided-shortlist best are scored by the error\n"
            "                           itself; runs in front of --reassign-tiles, --tile-moves and --tile-dither; with --backdrop-fixed the\n"
            "                           backdrop slot is passed by; not with --share, --devices or --nes.  The calls of a guided sweep go\n"
            "                           through the launch sets of --window like the scheduled ones (same result for every --window)\n"
            "      --guided-shortlist <K>  colours scored per guided call, 1..64 [default: 16: a choice, not a measurement]; needs --guided\n"
            "      --guided-proxy <PROXY>  the distance that ranks the colours: redmean, or cielab (CIEDE2000, the distance the pixels choose\n"
            "                           their entry by under --perceptual-palettes) [default: redmean]; needs --guided\n"
            "      --set-guided <G>     with --share: behind every G sweeps of the palette, one guided sweep of the set: the colours are ranked\n"
            "                           over the tiles of all frames, every frame scores the --set-guided-shortlist best, and the set's error\n"
            "                           decides; runs in front of --reassign-tiles, --tile-moves and --set-tile-dither; with\n"
            "                           --set-backdrop-fixed the backdrop slot is passed by; not with --devices or --nes.  The calls of a guided\n"
            "                           sweep of the set go through the launch sets of --window (same result for every --window)\n"
            "      --set-guided-shortlist <K>  colours scored per guided call of the set, 1..64 [default: 16: a choice, not a measurement];\n"
            "                           needs --set-guided\n"
            "      --set-guided-proxy <PROXY>  the same choice for the guided sweeps of the set: redmean or cielab [default: redmean];\n"
            "                           needs --set-guided\n"
            "      --max-tiles <N>      after the last optimizer call, merge tiles until at most N distinct characters are left (tiles equal\n"
            "                           under the tilemap's flips count once); each merge is the one with the lowest error among the\n"
            "                           --merge-shortlist cheapest by colour distance; not with --share or --devices\n"
            "      --merge-shortlist <K>  merges scored per step, 1..64 [default: 16: a choice, not a measurement]; needs --max-tiles\n"
            "                           or --max-set-tiles\n"
            "      --refit-tiles <N>    behind --max-tiles (or the last optimizer call), up to N sweeps (1..16) that refit every shared character\n"
            "                           to all the tiles using it and keep a refit where the error falls; stops after a sweep that accepts\n"
            "                           nothing; not with --share or --devices\n"
            "      --tilemap <F>        write the distinct characters and the tilemap (character, hflip, vflip, palette per tile) as JSON;\n"
            "                           not with --share or --devices\n"
            "      --max-set-tiles <N>  with --share: after the last optimizer call, merge tiles until the frames of the set hold at most N\n"
            "                           distinct characters together (1..8192; one VRAM character area for all frames): a tile may take\n"
            "                           its indices from a tile of another frame; at most 8192 tiles in all; not with --devices\n"
            "      --set-tilemap <F>    with --share: write the set's distinct characters and one tilemap per frame as JSON\n"
            "      --refit-set-tiles <N>  with --share: behind --max-set-tiles (or the last optimizer call), up to N sweeps (1..16) that refit\n"
            "                           every character shared across the frames to all the tiles using it and keep a refit where the\n"
            "                           set's error falls (one frame's error may rise); stops after a sweep that accepts nothing; not\n"
            "                           with --devices\n"
            "      --export-cgram <F>, --export-chr <F>, --export-map <F>\n"
            "                           write the result as the console loads it (any subset): the 512-byte CGRAM image, the distinct\n"
            "                           characters as bitplane data and the tilemap words of one 32-tile-wide screen; the bytes are\n"
            "                           rendered back and compared with the result before anything is written; not with --share or --devices\n"
            "      --set-export-cgram <F>, --set-export-chr <F>, --set-export-map <F>\n"
            "                           with --share: the same for the set: one CGRAM, one character area for all frames, and the frames'\n"
            "                           tilemaps one after another in member order; not with --devices or --set-backdrop(-fixed)\n"
            "      --export-bpp <2|4|8> depth of the exported characters [default: the smallest that holds the subpalette size]; 8 needs one\n"
            "                           subpalette; needs an export file\n"
            "      --export-char-base <N>  number of the first exported character in the tilemap words, 0..1023 [default: 0]\n"
            "      --export-palette-base <N>  CGRAM palette of subpalette 0, 0..7 [default: 0]\n"
            "      --export-priority <0|1>  priority bit of every tilemap word [default: 0]\n"
            "      --import-cgram <F>, --import-chr <F>, --import-map <F>\n"
            "                           start from native data instead of the k-means initialisers (all three are required): a 512-byte\n"
            "                           CGRAM image, bitplane characters and one tilemap word per tile, as the --export- options write\n"
            "                           them or as ripped from a ROM; the library refuses data the picture cannot hold and names the\n"
            "                           first such tile.  With --calls 0 the imported state itself is written (JSON, --preview, --tilemap,\n"
            "                           the --export- files), after --max-tiles and --refit-tiles if given: a reduced result can be\n"
            "                           reduced further.  With --calls N > 0 the first call's optimize() replaces the imported map, as it\n"
            "                           replaces every stored map: palette and tile palettes are what such a run continues from.  With\n"
            "                           --backdrop the backdrop colour is CGRAM word 0.  Not with --resume, --tile-palettes, --devices,\n"
            "                           --share or --backdrop-fixed\n"
            "      --set-import-cgram <F>, --set-import-chr <F>, --set-import-map <F>\n"
            "                           with --share: the same for the set: one CGRAM, one character area, and the frames' tilemaps one\n"
            "                           after another as --set-export-map writes them; not with --devices, --set-backdrop(-fixed) or --resume\n"
            "      --import-bpp <2|4|8> depth of the imported characters [default: the smallest that holds the subpalette size]; needs the\n"
            "                           import files\n"
            "      --import-char-base <N>  number of the first imported character in the tilemap words, 0..1023 [default: 0]\n"
            "      --import-palette-base <N>  CGRAM palette of subpalette 0 in the imported data, 0..7 [default: 0]\n"
            "      --share <S=T>        optimize one palette for the source and image S together (repeatable); S is decoded like the\n"
            "                           source and must have its size; its JSON goes to T, with the same palette as <TARGET_FILENAME>;\n"
            "                           --window 0 (several calls per launch set, sized by the library) or 1 (call by call) only;\n"
            "                           with --set-guided any --window: at most that many calls per launch set\n"
            "      --decode-only        write the decoded source as raw RGBA8 to <TARGET_FILENAME> and stop (no GPU)\n  -h, --help\n  -V, --version\n");
}
// the flat integer array stored under `"key":[...]` in one of this driver's (or the reference's) JSON outputs
bool json_int_array(const std::string &path, const char *key, std::vector<long> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string text; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const std::string pat = std::string("\"") + key + "\"";
    size_t at = text.find(pat);
    if (at == std::string::npos) return false;
    at = text.find('[', at + pat.size());
    if (at == std::string::npos) return false;
    out.clear();
    for (size_t i = at + 1; i < text.size(); ) {
        const char ch = text[i];
        if (ch == ']') return true;
        if (ch == '-' || (ch >= '0' && ch <= '9')) { char *end = nullptr; out.push_back(strtol(text.c_str() + i, &end, 10)); i = (size_t)(end - text.c_str()); }
        else if (ch == ',' || ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t') i++;
        else return false; // nested arrays or anything else: not a flat integer array
    }
    return false;
}
// the integer stored under `"key":N`
bool json_int_scalar(const std::string &path, const char *key, long &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string text; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const std::string pat = std::string("\"") + key + "\"";
    size_t at = text.find(pat);
    if (at == std::string::npos) return false;
    at = text.find(':', at + pat.size());
    if (at == std::string::npos) return false;
    char *end = nullptr;
    out = strtol(text.c_str() + at + 1, &end, 10);
    return end != text.c_str() + at + 1;
}

// the arrays of integers stored under `"key":[[...],[...]]`
bool json_int_arrays(const std::string &path, const char *key, std::vector<std::vector<long>> &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string text; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const std::string pat = std::string("\"") + key + "\"";
    size_t at = text.find(pat);
    if (at == std::string::npos) return false;
    at = text.find('[', at + pat.size());
    if (at == std::string::npos) return false;
    out.clear();
    bool inner = false;
    for (size_t i = at + 1; i < text.size(); ) {
        const char ch = text[i];
        if (ch == '[' && !inner) { inner = true; out.emplace_back(); i++; }
        else if (ch == ']' && inner) { inner = false; i++; }
        else if (ch == ']') return true;
        else if (inner && (ch == '-' || (ch >= '0' && ch <= '9'))) { char *end = nullptr; out.back().push_back(strtol(text.c_str() + i, &end, 10)); i = (size_t)(end - text.c_str()); }
        else if (ch == ',' || ch == ' ' || ch == '\n' || ch == '\r' || ch == '\t') i++;
        else return false;
    }
    return false;
}
// the boolean stored under `"key":true|false`
bool json_bool(const std::string &path, const char *key, bool &out) {
    FILE *f = fopen(path.c_str(), "rb");
    if (!f) return false;
    std::string text; char buf[65536]; size_t n;
    while ((n = fread(buf, 1, sizeof buf, f)) > 0) text.append(buf, n);
    fclose(f);
    const std::string pat = std::string("\"") + key + "\"";
    size_t at = text.find(pat);
    if (at == std::string::npos) return false;
    at = text.find(':', at + pat.size());
    if (at == std::string::npos) return false;
    at++;
    while (at < text.size() && (text[at] == ' ' || text[at] == '\n' || text[at] == '\r' || text[at] == '\t')) at++;
    if (text.compare(at, 4, "true") == 0) { out = true; return true; }
    if (text.compare(at, 5, "false") == 0) { out = false; return true; }
    return false;
}

void synth(uint64_t seed, uint32_t w, uint32_t h, std::vector<uint8_t> &out) {
    out.resize((size_t)w * h * 4);
    uint64_t s = seed;
    for (uint32_t y = 0; y < h; y++)
        for (uint32_t x = 0; x < w; x++) {
            uint64_t z = (s += 0x9E3779B97F4A7C15ull);
            z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
            z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
            z ^= z >> 31;
            uint8_t *o = &out[4 * ((size_t)y * w + x)];
            o[0] = (uint8_t)(x + (z & 63)); o[1] = (uint8_t)(y + ((z >> 8) & 63)); o[2] = (uint8_t)((x + y) / 2 + ((z >> 16) & 63)); o[3] = 255;
        }
}

// the source image: PNG, raw RGBA8 (256 x H x 4 bytes) or synth:SEED
void load_source(const std::string &source, uint32_t &w, uint32_t &h, std::vector<uint8_t> &rgba) {
    w = 256; h = 256;
    if (source.rfind("synth:", 0) == 0) synth(strtoull(source.c_str() + 6, nullptr, 0), w, h, rgba);
    else {
        FILE *f = fopen(source.c_str(), "rb");
        if (!f) die("No such file or directory: " + source);
        fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> file(n > 0 ? (size_t)n : 0);
        if (n <= 0 || fread(file.data(), 1, (size_t)n, f) != (size_t)n) { fclose(f); die("short read on " + source); }
        fclose(f);
        if (snes_png::is_png(file.data(), file.size())) {
            std::string err;
            if (!snes_png::decode(file.data(), file.size(), w, h, rgba, err)) die("Format error decoding Png: " + err);
            // src/lib.rs:838-840 tests `width != 256 && height != 256` and then indexes tiles with a hard-coded 32;
            // this build admits what that arithmetic handles: 256 wide, and the height the library accepts
            if (w != 256) die("Image size must be 256x256");
        } else {
            if (n % (256 * 4) != 0) die("Image size must be 256x256"); // src/lib.rs:838-840
            h = (uint32_t)(n / (256 * 4));
            rgba.swap(file);
        }
    }
}

void write_json(snesimage_ctx *ctx, const std::string &target) { // src/lib.rs:1000-1002
    int64_t need = snesimage_as_json(ctx, nullptr, 0);
    if (need < 0) die(snesimage_last_error());
    std::vector<char> json((size_t)need);
    snesimage_as_json(ctx, json.data(), need);
    FILE *f = fopen(target.c_str(), "wb");
    if (!f) die("cannot create " + target);
    fwrite(json.data(), 1, (size_t)need - 1, f);
    fclose(f);
}

// The flags of guided sweeps, a context's (--guided*) or a set's (--set-guided*): one sweep behind every G, the shortlist, the proxy.
struct GuidedFlags {
    uint32_t every = 0, shortlist = 16, proxy = SNES_GUIDE_REDMEAN;
    bool given = false, short_given = false, proxy_given = false;
    std::string arg, short_arg, proxy_arg;
    bool any() const { return given || short_given || proxy_given; }
    const char *proxy_name() const { return proxy == SNES_GUIDE_CIELAB ? "cielab" : "redmean"; }
};
// Checks and parses them: n is "--guided" or "--set-guided", refusal what else rules the sweeps out (its place is behind the
// proxy's name and before the numbers), or empty.  False: the error has been said.
bool parse_guided(const char *n, GuidedFlags &f, const std::string &refusal) {
    if (!f.given && f.short_given) { fprintf(stderr, "error: '%s-shortlist <K>' needs '%s <G>'\n", n, n); return false; }
    if (!f.given) { fprintf(stderr, "error: '%s-proxy <PROXY>' needs '%s <G>'\n", n, n); return false; }
    if (f.proxy_given) {
        if (f.proxy_arg != "redmean" && f.proxy_arg != "cielab") { fprintf(stderr, "error: invalid value '%s' for '%s-proxy <PROXY>': expected redmean or cielab\n", f.proxy_arg.c_str(), n); return false; }
        f.proxy = f.proxy_arg == "cielab" ? SNES_GUIDE_CIELAB : SNES_GUIDE_REDMEAN;
    }
    if (!refusal.empty()) { fprintf(stderr, "error: %s\n", refusal.c_str()); return false; }
    char *end = nullptr;
    const unsigned long g = strtoul(f.arg.c_str(), &end, 10);
    if (f.arg.empty() || f.arg[0] == '-' || *end || g < 1 || g > 1000000) { fprintf(stderr, "error: invalid value '%s' for '%s <G>': expected a number of sweeps, 1 or more\n", f.arg.c_str(), n); return false; }
    f.every = (uint32_t)g;
    if (f.short_given) {
        const unsigned long k = strtoul(f.short_arg.c_str(), &end, 10);
        if (f.short_arg.empty() || f.short_arg[0] == '-' || *end || k < 1 || k > 64) { fprintf(stderr, "error: invalid value '%s' for '%s-shortlist <K>': expected 1..64\n", f.short_arg.c_str(), n); return false; }
        f.shortlist = (uint32_t)k;
    }
    return true;
}

} // namespace

int main(int argc, char **argv) {
    std::vector<std::string> pos;
    uint32_t count = 1, size = 7, flags = 0, calls = 0, ncand = 64, reassign_every = 0, tile_every = 0, window = 0; // src/config.rs:13-18 defaults
    uint64_t seed = 1;
    int device = 0;
    std::string tile_file, preview_file, resume_file, tilemap_file, max_tiles_arg, merge_short_arg, refit_arg, set_tilemap_file, max_set_arg, refit_set_arg;
    bool max_tiles_given = false, merge_short_given = false, refit_given = false, max_set_given = false, refit_set_given = false; uint32_t max_tiles = 0, merge_short = 0, refit_sweeps = 0, max_set_tiles = 0, refit_set_sweeps = 0;
    std::vector<int> devices; // --devices: candidate sharding over several GPUs from this one process
    std::vector<std::pair<std::string, std::string>> shares; // --share SOURCE=TARGET: images optimized with the source's palette
    bool decode_only = false;
    bool blocks_given = false; std::string blocks_arg; uint32_t blocks_w = 1, blocks_h = 1; // --palette-blocks WxH
    uint32_t ordered_n = 0, ordered_amp = 32; bool ordered_given = false, amp_given = false; std::string ordered_arg, amp_arg;
    bool backdrop = false, backdrop_fixed = false; uint8_t backdrop_rgb[3] = {0, 0, 0}; std::string backdrop_arg;
    bool set_backdrop = false, set_backdrop_fixed = false; std::string set_backdrop_arg; // the backdrop colour of a --share set
    uint32_t level_every = 0, dither_levels = 4; bool level_given = false, dither_levels_given = false; std::string level_arg, dither_levels_arg, levels_out_file, levels_in_file;
    uint32_t set_level_every = 0; bool set_level_given = false, set_mode_given = false, set_tied = true; std::string set_level_arg, set_mode_arg, set_levels_out_file, set_levels_in_file;
    GuidedFlags gd, sgd; // --guided*, --set-guided*
    std::string export_file[3], set_export_file[3]; // --export-cgram / -chr / -map and their --set- kin
    struct { const char *name, *shown; bool given; std::string arg; unsigned long lo, hi, value; } export_opt[4] = { // the layout of whichever family is present
        {"--export-bpp", "--export-bpp <2|4|8>", false, "", 2, 8, 0}, {"--export-char-base", "--export-char-base <N>", false, "", 0, 1023, 0},
        {"--export-palette-base", "--export-palette-base <N>", false, "", 0, 7, 0}, {"--export-priority", "--export-priority <0|1>", false, "", 0, 1, 0}};
    std::string import_file[3], set_import_file[3]; // --import-cgram / -chr / -map and their --set- kin
    struct { const char *name, *shown; bool given; std::string arg; unsigned long lo, hi, value; } import_opt[3] = { // what the imported files are laid out as
        {"--import-bpp", "--import-bpp <2|4|8>", false, "", 2, 8, 0}, {"--import-char-base", "--import-char-base <N>", false, "", 0, 1023, 0},
        {"--import-palette-base", "--import-palette-base <N>", false, "", 0, 7, 0}};
    static const char *const kImportName[3] = {"--import-cgram", "--import-chr", "--import-map"}, *const kSetImportName[3] = {"--set-import-cgram", "--set-import-chr", "--set-import-map"};
    static const char *const kExportName[3] = {"--export-cgram", "--export-chr", "--export-map"}, *const kSetExportName[3] = {"--set-export-cgram", "--set-export-chr", "--set-export-map"};
    for (int i = 1; i < argc; i++) {
        std::string a = argv[i];
        auto need = [&](const char *name) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '%s'\n", name); exit(2); } return argv[++i]; };
        if (a == "-c" || a == "--subpalette-count") count = (uint32_t)strtoul(need("--subpalette-count"), nullptr, 10);
        else if (a == "-s" || a == "--subpalette-size") size = (uint32_t)strtoul(need("--subpalette-size"), nullptr, 10);
        else if (a == "-d" || a == "--dither") flags |= SNES_DITHER;
        else if (a == "--perceptual-palettes") flags |= SNES_PERCEPTUAL;
        else if (a == "--nes") flags |= SNES_NES;
        else if (a == "--backdrop") backdrop = true;
        else if (a == "--backdrop-fixed") { backdrop_fixed = true; backdrop_arg = need("--backdrop-fixed"); }
        else if (a == "--set-backdrop") set_backdrop = true;
        else if (a == "--set-backdrop-fixed") { set_backdrop_fixed = true; set_backdrop_arg = need("--set-backdrop-fixed"); }
        else if (a == "--ordered-dither") { ordered_given = true; ordered_arg = need("--ordered-dither"); }
        else if (a == "--dither-amplitude") { amp_given = true; amp_arg = need("--dither-amplitude"); }
        else if (a == "--tile-dither") { level_given = true; level_arg = need("--tile-dither"); }
        else if (a == "--dither-levels") { dither_levels_given = true; dither_levels_arg = need("--dither-levels"); }
        else if (a == "--tile-levels-out") levels_out_file = need("--tile-levels-out");
        else if (a == "--tile-levels-in") levels_in_file = need("--tile-levels-in");
        else if (a == "--set-tile-dither") { set_level_given = true; set_level_arg = need("--set-tile-dither"); }
        else if (a == "--set-levels") { set_mode_given = true; set_mode_arg = need("--set-levels"); }
        else if (a == "--set-tile-levels-out") set_levels_out_file = need("--set-tile-levels-out");
        else if (a == "--set-tile-levels-in") set_levels_in_file = need("--set-tile-levels-in");
        else if (a == "--calls") calls = (uint32_t)strtoul(need("--calls"), nullptr, 10);
        else if (a == "--candidates") ncand = (uint32_t)strtoul(need("--candidates"), nullptr, 10);
        else if (a == "--seed") seed = strtoull(need("--seed"), nullptr, 0);
        else if (a == "--window") window = (uint32_t)strtoul(need("--window"), nullptr, 10);
        else if (a == "--device") device = atoi(need("--device"));
        else if (a == "--devices") { for (const char *q = need("--devices"); *q;) { char *end = nullptr; devices.push_back((int)strtol(q, &end, 10)); if (end == q) { fprintf(stderr, "error: invalid value for '--devices'\n"); return 2; } q = *end == ',' ? end + 1 : end; } }
        else if (a == "--tile-palettes") tile_file = need("--tile-palettes");
        else if (a == "--preview") preview_file = need("--preview");
        else if (a == "--reassign-tiles") reassign_every = (uint32_t)strtoul(need("--reassign-tiles"), nullptr, 10);
        else if (a == "--tile-moves") tile_every = (uint32_t)strtoul(need("--tile-moves"), nullptr, 10);
        else if (a == "--resume") resume_file = need("--resume");
        else if (a == "--palette-blocks") { blocks_given = true; blocks_arg = need("--palette-blocks"); }
        else if (a == "--guided") { gd.given = true; gd.arg = need("--guided"); }
        else if (a == "--guided-shortlist") { gd.short_given = true; gd.short_arg = need("--guided-shortlist"); }
        else if (a == "--guided-proxy") { gd.proxy_given = true; gd.proxy_arg = need("--guided-proxy"); }
        else if (a == "--set-guided-proxy") { sgd.proxy_given = true; sgd.proxy_arg = need("--set-guided-proxy"); }
        else if (a == "--set-guided") { sgd.given = true; sgd.arg = need("--set-guided"); }
        else if (a == "--set-guided-shortlist") { sgd.short_given = true; sgd.short_arg = need("--set-guided-shortlist"); }
        else if (a == "--max-tiles") { max_tiles_given = true; max_tiles_arg = need("--max-tiles"); }
        else if (a == "--merge-shortlist") { merge_short_given = true; merge_short_arg = need("--merge-shortlist"); }
        else if (a == "--refit-tiles") { refit_given = true; refit_arg = need("--refit-tiles"); }
        else if (a == "--tilemap") tilemap_file = need("--tilemap");
        else if (a == "--max-set-tiles") { max_set_given = true; max_set_arg = need("--max-set-tiles"); }
        else if (a == "--set-tilemap") set_tilemap_file = need("--set-tilemap");
        else if (a == "--refit-set-tiles") { refit_set_given = true; refit_set_arg = need("--refit-set-tiles"); }
        else if (a == "--export-cgram" || a == "--export-chr" || a == "--export-map") { for (int k = 0; k < 3; k++) if (a == kExportName[k]) export_file[k] = need(kExportName[k]); }
        else if (a == "--set-export-cgram" || a == "--set-export-chr" || a == "--set-export-map") { for (int k = 0; k < 3; k++) if (a == kSetExportName[k]) set_export_file[k] = need(kSetExportName[k]); }
        else if (a == "--export-bpp" || a == "--export-char-base" || a == "--export-palette-base" || a == "--export-priority") {
            for (auto &o : export_opt) if (a == o.name) { o.given = true; o.arg = need(o.name); }
        }
        else if (a == "--import-cgram" || a == "--import-chr" || a == "--import-map") { for (int k = 0; k < 3; k++) if (a == kImportName[k]) import_file[k] = need(kImportName[k]); }
        else if (a == "--set-import-cgram" || a == "--set-import-chr" || a == "--set-import-map") { for (int k = 0; k < 3; k++) if (a == kSetImportName[k]) set_import_file[k] = need(kSetImportName[k]); }
        else if (a == "--import-bpp" || a == "--import-char-base" || a == "--import-palette-base") {
            for (auto &o : import_opt) if (a == o.name) { o.given = true; o.arg = need(o.name); }
        }
        else if (a == "--share") {
            const std::string v = need("--share");
            const size_t eq = v.find('=');
            if (eq == std::string::npos || eq == 0 || eq + 1 == v.size()) { fprintf(stderr, "error: invalid value '%s' for '--share <SOURCE=TARGET>': expected SOURCE=TARGET\n", v.c_str()); return 2; }
            shares.emplace_back(v.substr(0, eq), v.substr(eq + 1));
        }
        else if (a == "--decode-only") decode_only = true;
        else if (a == "-h" || a == "--help") { usage(); return 0; }
        else if (a == "-V" || a == "--version") { printf("snesimage 0.1.1 (%s)\n", snesimage_version()); return 0; }
        else if (!a.empty() && a[0] == '-' && a != "-") { fprintf(stderr, "error: unexpected argument '%s' found\n", a.c_str()); usage(); return 2; }
        else pos.push_back(a);
    }
    if (tile_every) { // objective-scored moves and the colour-distance proxy undo each other; no group entry point for the moves
        const char *bad = !devices.empty() ? "'--devices'" : (reassign_every ? "'--reassign-tiles'" : nullptr);
        if (bad) { fprintf(stderr, "error: the argument '--tile-moves <K>' cannot be used with %s\n", bad); return 2; }
    }
    if (gd.any()) { // guided sweeps: said before any file or device is touched
        const char *bad = !shares.empty() ? "'--share'" : !devices.empty() ? "'--devices'" : (flags & SNES_NES) ? "'--nes'" : nullptr; // one context of its own; the NES call scores its whole table already
        if (!parse_guided("--guided", gd, bad ? std::string("the argument '--guided <G>' cannot be used with ") + bad : "")) return 2;
    }
    if (sgd.any()) { // guided sweeps of a set: said before any file or device is touched
        const char *bad = !devices.empty() ? "'--devices'" : (flags & SNES_NES) ? "'--nes'" : nullptr; // a set runs on one device; the NES call scores its whole table already
        if (!parse_guided("--set-guided", sgd, shares.empty() ? "'--set-guided <G>' needs '--share <SOURCE=TARGET>': it runs the guided sweeps of a set (one image: --guided)"
                                               : bad ? std::string("the argument '--set-guided <G>' cannot be used with ") + bad : "")) return 2;
    }
    if (max_tiles_given || merge_short_given || refit_given || !tilemap_file.empty()) { // said before any file or device is touched
        char *end = nullptr;
        if (merge_short_given && !max_tiles_given && !max_set_given) { fprintf(stderr, "error: '--merge-shortlist <K>' needs '--max-tiles <N>' or '--max-set-tiles <N>'\n"); return 2; }
        const char *opt = max_tiles_given ? "--max-tiles <N>" : (refit_given ? "--refit-tiles <N>" : "--tilemap <F>");
        const char *bad = !shares.empty() ? "'--share'" : (!devices.empty() ? "'--devices'" : nullptr); // characters are counted in one image on one device
        if (bad && (max_tiles_given || refit_given || !tilemap_file.empty())) { fprintf(stderr, "error: the argument '%s' cannot be used with %s\n", opt, bad); return 2; }
        if (max_tiles_given) {
            const unsigned long n = strtoul(max_tiles_arg.c_str(), &end, 10);
            if (max_tiles_arg.empty() || *end || n < 1 || n > 1024) { fprintf(stderr, "error: invalid value '%s' for '--max-tiles <N>': expected 1..1024\n", max_tiles_arg.c_str()); return 2; }
            max_tiles = (uint32_t)n;
        }
        if (merge_short_given) {
            const unsigned long k = strtoul(merge_short_arg.c_str(), &end, 10);
            if (merge_short_arg.empty() || *end || k < 1 || k > 64) { fprintf(stderr, "error: invalid value '%s' for '--merge-shortlist <K>': expected 1..64\n", merge_short_arg.c_str()); return 2; }
            merge_short = (uint32_t)k;
        }
        if (refit_given) {
            const unsigned long n = strtoul(refit_arg.c_str(), &end, 10);
            if (refit_arg.empty() || *end || n < 1 || n > 16) { fprintf(stderr, "error: invalid value '%s' for '--refit-tiles <N>': expected 1..16\n", refit_arg.c_str()); return 2; }
            refit_sweeps = (uint32_t)n;
        }
    }
    if (max_set_given || !set_tilemap_file.empty()) { // the budget of a set: said before any file or device is touched
        const char *opt = max_set_given ? "--max-set-tiles <N>" : "--set-tilemap <F>";
        if (shares.empty()) { fprintf(stderr, "error: '%s' needs '--share <SOURCE=TARGET>': it counts the characters of a set (one image: --max-tiles, --tilemap)\n", opt); return 2; }
        if (!devices.empty()) { fprintf(stderr, "error: the argument '%s' cannot be used with '--devices'\n", opt); return 2; }
        if (max_set_given) {
            char *end = nullptr;
            const unsigned long n = strtoul(max_set_arg.c_str(), &end, 10);
            if (max_set_arg.empty() || *end || n < 1 || n > 8192) { fprintf(stderr, "error: invalid value '%s' for '--max-set-tiles <N>': expected 1..8192\n", max_set_arg.c_str()); return 2; }
            max_set_tiles = (uint32_t)n;
        }
    }
    if (refit_set_given) { // the refit of a set: said before any file or device is touched
        if (shares.empty()) { fprintf(stderr, "error: '--refit-set-tiles <N>' needs '--share <SOURCE=TARGET>': it refits the characters of a set (one image: --refit-tiles)\n"); return 2; }
        if (!devices.empty()) { fprintf(stderr, "error: the argument '--refit-set-tiles <N>' cannot be used with '--devices'\n"); return 2; }
        char *end = nullptr;
        const unsigned long n = strtoul(refit_set_arg.c_str(), &end, 10);
        if (refit_set_arg.empty() || refit_set_arg[0] == '-' || *end || n < 1 || n > 16) { fprintf(stderr, "error: invalid value '%s' for '--refit-set-tiles <N>': expected 1..16\n", refit_set_arg.c_str()); return 2; }
        refit_set_sweeps = (uint32_t)n;
    }
    int export_first = -1, set_export_first = -1; // the first export file of each family that was given
    for (int k = 2; k >= 0; k--) { if (!export_file[k].empty()) export_first = k; if (!set_export_file[k].empty()) set_export_first = k; }
    { // the native export: said before any file or device is touched
        if (export_first >= 0) {
            const char *bad = !shares.empty() ? "'--share'" : (!devices.empty() ? "'--devices'" : nullptr); // characters are counted in one image on one device
            if (bad) { fprintf(stderr, "error: the argument '%s <F>' cannot be used with %s\n", kExportName[export_first], bad); return 2; }
        }
        if (set_export_first >= 0) {
            const char *opt = kSetExportName[set_export_first];
            if (shares.empty()) { fprintf(stderr, "error: '%s <F>' needs '--share <SOURCE=TARGET>': it exports the characters of a set (one image: --export-cgram, --export-chr, --export-map)\n", opt); return 2; }
            const char *bad = !devices.empty() ? "'--devices'" : set_backdrop ? "'--set-backdrop'" : set_backdrop_fixed ? "'--set-backdrop-fixed'" : nullptr; // a backdrop set has no character calls yet
            if (bad) { fprintf(stderr, "error: the argument '%s <F>' cannot be used with %s\n", opt, bad); return 2; }
        }
        for (auto &o : export_opt) {
            if (!o.given) continue;
            if (export_first < 0 && set_export_first < 0) { fprintf(stderr, "error: '%s' needs an export file: '--export-cgram', '--export-chr', '--export-map' or, with --share, their '--set-export-' kin\n", o.shown); return 2; }
            char *end = nullptr;
            o.value = strtoul(o.arg.c_str(), &end, 10);
            const bool is_bpp = std::string(o.name) == "--export-bpp";
            if (o.arg.empty() || o.arg[0] == '-' || *end || o.value < o.lo || o.value > o.hi || (is_bpp && o.value != 2 && o.value != 4 && o.value != 8)) {
                if (is_bpp) fprintf(stderr, "error: invalid value '%s' for '%s': expected 2, 4 or 8\n", o.arg.c_str(), o.shown);
                else fprintf(stderr, "error: invalid value '%s' for '%s': expected %lu..%lu\n", o.arg.c_str(), o.shown, o.lo, o.hi);
                return 2;
            }
        }
    }
    int import_first = -1, set_import_first = -1; // the first import file of each family that was given
    for (int k = 2; k >= 0; k--) { if (!import_file[k].empty()) import_first = k; if (!set_import_file[k].empty()) set_import_first = k; }
    { // the native import: said before any file or device is touched
        if (import_first >= 0) {
            const char *opt = kImportName[import_first];
            for (int k = 0; k < 3; k++) if (import_file[k].empty()) { fprintf(stderr, "error: '%s <F>' needs '%s <F>': a state is CGRAM, characters and tilemap words together\n", opt, kImportName[k]); return 2; }
            const char *bad = !resume_file.empty() ? "'--resume'" : !tile_file.empty() ? "'--tile-palettes'" : !devices.empty() ? "'--devices'" : !shares.empty() ? "'--share'"
                            : backdrop_fixed ? "'--backdrop-fixed'" : nullptr; // one state for one image on one device; the backdrop colour is the file's
            if (bad) { fprintf(stderr, "error: the argument '%s <F>' cannot be used with %s\n", opt, bad); return 2; }
        }
        if (set_import_first >= 0) {
            const char *opt = kSetImportName[set_import_first];
            if (shares.empty()) { fprintf(stderr, "error: '%s <F>' needs '--share <SOURCE=TARGET>': it imports the state of a set (one image: --import-cgram, --import-chr, --import-map)\n", opt); return 2; }
            for (int k = 0; k < 3; k++) if (set_import_file[k].empty()) { fprintf(stderr, "error: '%s <F>' needs '%s <F>': a state is CGRAM, characters and tilemap words together\n", opt, kSetImportName[k]); return 2; }
            const char *bad = !devices.empty() ? "'--devices'" : set_backdrop ? "'--set-backdrop'" : set_backdrop_fixed ? "'--set-backdrop-fixed'" : !resume_file.empty() ? "'--resume'" : nullptr; // a backdrop set has no character calls yet
            if (bad) { fprintf(stderr, "error: the argument '%s <F>' cannot be used with %s\n", opt, bad); return 2; }
        }
        for (auto &o : import_opt) {
            if (!o.given) continue;
            if (import_first < 0 && set_import_first < 0) { fprintf(stderr, "error: '%s' needs the import files: '--import-cgram', '--import-chr' and '--import-map' or, with --share, their '--set-import-' kin\n", o.shown); return 2; }
            char *end = nullptr;
            o.value = strtoul(o.arg.c_str(), &end, 10);
            const bool is_bpp = std::string(o.name) == "--import-bpp";
            if (o.arg.empty() || o.arg[0] == '-' || *end || o.value < o.lo || o.value > o.hi || (is_bpp && o.value != 2 && o.value != 4 && o.value != 8)) {
                if (is_bpp) fprintf(stderr, "error: invalid value '%s' for '%s': expected 2, 4 or 8\n", o.arg.c_str(), o.shown);
                else fprintf(stderr, "error: invalid value '%s' for '%s': expected %lu..%lu\n", o.arg.c_str(), o.shown, o.lo, o.hi);
                return 2;
            }
        }
    }
    if (blocks_given) { // palette blocks: said before any file or device is touched (the height is judged once the image is read)
        const char *bad = !shares.empty() ? "--share" : !devices.empty() ? "--devices" : import_first >= 0 ? kImportName[import_first] : set_import_first >= 0 ? kSetImportName[set_import_first] : nullptr;
        if (bad) { fprintf(stderr, "error: the argument '--palette-blocks <WxH>' cannot be used with '%s'\n", bad); return 2; }
        unsigned bw = 0, bh = 0; char tail = 0;
        auto ok = [](unsigned v) { return v == 1 || v == 2 || v == 4 || v == 8; };
        if (sscanf(blocks_arg.c_str(), "%ux%u%c", &bw, &bh, &tail) != 2 || !ok(bw) || !ok(bh)) {
            fprintf(stderr, "error: invalid value '%s' for '--palette-blocks <WxH>': expected W and H of 1, 2, 4 or 8 tiles, such as 2x2\n", blocks_arg.c_str()); return 2; }
        blocks_w = bw; blocks_h = bh;
    }
    if (pos.size() != 2) { fprintf(stderr, "error: the following required arguments were not provided: <SOURCE_FILENAME> <TARGET_FILENAME>\n"); usage(); return 2; }
    const std::string source = pos[0], target = pos[1];
    const bool set_bd = set_backdrop || set_backdrop_fixed;
    if (set_bd) { // the backdrop colour of a set: said before any file or device is touched
        const char *opt = set_backdrop_fixed ? "--set-backdrop-fixed <R,G,B>" : "--set-backdrop";
        if (shares.empty()) { fprintf(stderr, "error: '%s' needs '--share <SOURCE=TARGET>': it carries the backdrop colour of a set (one image: --backdrop)\n", opt); return 2; }
        const char *bad = !devices.empty() ? "'--devices'" : backdrop ? "'--backdrop'" : backdrop_fixed ? "'--backdrop-fixed'" : (set_backdrop && set_backdrop_fixed) ? "'--set-backdrop-fixed'"
                        : max_set_given ? "'--max-set-tiles'" : refit_set_given ? "'--refit-set-tiles'" : !set_tilemap_file.empty() ? "'--set-tilemap'"
                        : set_level_given ? "'--set-tile-dither'" : set_mode_given ? "'--set-levels'" : !set_levels_out_file.empty() ? "'--set-tile-levels-out'" : !set_levels_in_file.empty() ? "'--set-tile-levels-in'" : nullptr;
        if (bad) { fprintf(stderr, "error: the argument '%s' cannot be used with %s\n", set_backdrop ? "--set-backdrop" : opt, bad); return 2; }
        if (set_backdrop_fixed) {
            unsigned v[3]; char tail = 0;
            if (sscanf(set_backdrop_arg.c_str(), "%u,%u,%u%c", &v[0], &v[1], &v[2], &tail) != 3 || v[0] > 31 || v[1] > 31 || v[2] > 31) {
                fprintf(stderr, "error: invalid value '%s' for '--set-backdrop-fixed <R,G,B>': expected three 5-bit values, such as 0,0,31\n", set_backdrop_arg.c_str()); return 2; }
            for (int k = 0; k < 3; k++) backdrop_rgb[k] = (uint8_t)v[k];
        }
        if (size > 15 || (unsigned long long)count * (size + 1) > 253) {
            fprintf(stderr, "error: '%s' needs --subpalette-size <= 15 and count * (size + 1) <= 253: a row of 16 colours holds the backdrop colour and 15 of its own\n", opt); return 2; }
        flags |= SNES_BACKDROP;
    }
    if (!shares.empty()) { // a set runs on one device, from the k-means initialisers (a backdrop set also from --resume); its windows are sized by the library (--window 0) or off (--window 1)
        const char *bad = (!resume_file.empty() && !set_bd) ? "'--resume'" : !devices.empty() ? "'--devices'" : !tile_file.empty() ? "'--tile-palettes'" : (window > 1 && !sgd.given ? "'--window' other than 0 or 1" : nullptr); // (with --set-guided the launch sets take at most --window calls)
        if (bad) { fprintf(stderr, "error: the argument '--share <SOURCE=TARGET>' cannot be used with %s\n", bad); return 2; }
    }
    if (ordered_given || amp_given) { // said before any device is touched
        char *end = nullptr;
        if (!ordered_given) { fprintf(stderr, "error: '--dither-amplitude <A>' needs '--ordered-dither <N>'\n"); return 2; }
        const unsigned long n = strtoul(ordered_arg.c_str(), &end, 10);
        if (ordered_arg.empty() || *end || (n != 2 && n != 4 && n != 8 && n != 16)) { fprintf(stderr, "error: invalid value '%s' for '--ordered-dither <N>': expected 2, 4, 8 or 16\n", ordered_arg.c_str()); return 2; }
        ordered_n = (uint32_t)n;
        if (amp_given) {
            const unsigned long amp = strtoul(amp_arg.c_str(), &end, 10);
            if (amp_arg.empty() || *end || amp < 1 || amp > 255) { fprintf(stderr, "error: invalid value '%s' for '--dither-amplitude <A>': expected 1..255\n", amp_arg.c_str()); return 2; }
            ordered_amp = (uint32_t)amp;
        }
        if (flags & SNES_DITHER) { fprintf(stderr, "error: the argument '--ordered-dither <N>' cannot be used with '--dither': they are alternatives\n"); return 2; }
    }
    int8_t ordered_tab[256] = {};
    if (ordered_n) snesimage_bayer_offsets(ordered_n, ordered_amp, ordered_tab);
    // per-tile levels: the ladder of amplitudes (level 0 = none, level j = A*j/(L-1)) or the one of --tile-levels-in
    std::vector<long> level_amps, levels_in;
    const bool set_level_opts = set_level_given || set_mode_given || !set_levels_out_file.empty() || !set_levels_in_file.empty(); // the levels of a set: their own options
    if (level_given || (dither_levels_given && !set_level_opts) || !levels_out_file.empty() || !levels_in_file.empty()) { // said before any file or device is touched
        const char *opt = level_given ? "--tile-dither <K>" : dither_levels_given ? "--dither-levels <L>" : !levels_out_file.empty() ? "--tile-levels-out <F>" : "--tile-levels-in <F>";
        const char *bad = (flags & SNES_DITHER) ? "'--dither'" : !shares.empty() ? "'--share'" : (!devices.empty() ? "'--devices'" : nullptr); // error diffusion has no levels; sets and groups share one table
        if (bad) { fprintf(stderr, "error: the argument '%s' cannot be used with %s\n", opt, bad); return 2; }
        if (!ordered_given) { fprintf(stderr, "error: '%s' needs '--ordered-dither <N>'\n", opt); return 2; }
        char *end = nullptr;
        if (level_given) {
            const unsigned long k = strtoul(level_arg.c_str(), &end, 10);
            if (level_arg.empty() || level_arg[0] == '-' || *end || k < 1 || k > 1000000) { fprintf(stderr, "error: invalid value '%s' for '--tile-dither <K>': expected a number of sweeps, 1 or more\n", level_arg.c_str()); return 2; }
            level_every = (uint32_t)k;
        }
        if (dither_levels_given) {
            const unsigned long l = strtoul(dither_levels_arg.c_str(), &end, 10);
            if (dither_levels_arg.empty() || *end || l < 2 || l > 8) { fprintf(stderr, "error: invalid value '%s' for '--dither-levels <L>': expected 2..8\n", dither_levels_arg.c_str()); return 2; }
            dither_levels = (uint32_t)l;
        }
        if (!level_given && levels_in_file.empty()) { fprintf(stderr, "error: '%s' needs '--tile-dither <K>' or '--tile-levels-in <F>'\n", opt); return 2; }
        if (levels_in_file.empty() && ordered_amp < dither_levels - 1) {
            fprintf(stderr, "error: '--dither-levels %u' needs '--dither-amplitude' of at least %u: every level is a different amplitude\n", dither_levels, dither_levels - 1); return 2; }
        if (!levels_in_file.empty()) {
            long n_in = 0;
            if (!json_int_scalar(levels_in_file, "n", n_in) || !json_int_array(levels_in_file, "amplitudes", level_amps) || !json_int_array(levels_in_file, "levels", levels_in))
                die("cannot read n, amplitudes and levels from " + levels_in_file);
            if (n_in != (long)ordered_n) die(levels_in_file + " was written for --ordered-dither " + std::to_string(n_in));
            if (level_amps.empty() || level_amps.size() > 8) die(levels_in_file + ": 1 to 8 amplitudes expected");
            for (long a : level_amps) if (a < 0 || a > 255) die(levels_in_file + ": amplitude out of range");
            for (long l : levels_in) if (l < 0 || l >= (long)level_amps.size()) die(levels_in_file + ": level out of range");
            // the ladder is the file's: a --dither-levels or --dither-amplitude that says otherwise is a mistake, not a preference
            if (dither_levels_given && dither_levels != level_amps.size()) die(levels_in_file + " holds " + std::to_string(level_amps.size()) + " levels, --dither-levels says " + std::to_string(dither_levels));
            const long top = *std::max_element(level_amps.begin(), level_amps.end());
            if (amp_given && (long)ordered_amp != top) die(levels_in_file + " was written for --dither-amplitude " + std::to_string(top) + ", the command line says " + std::to_string(ordered_amp));
            ordered_amp = (uint32_t)top; // (what the log reports)
        } else for (uint32_t j = 0; j < dither_levels; j++) level_amps.push_back((long)(ordered_amp * j / (dither_levels - 1)));
    }
    std::vector<std::vector<long>> set_levels_in; // --set-tile-levels-in: one list of levels per frame
    if (set_level_opts) { // said before any file or device is touched
        const char *opt = set_level_given ? "--set-tile-dither <K>" : set_mode_given ? "--set-levels <tied|frame>" : !set_levels_out_file.empty() ? "--set-tile-levels-out <F>" : "--set-tile-levels-in <F>";
        const char *bad = (flags & SNES_DITHER) ? "'--dither'" : (!devices.empty() ? "'--devices'" : (level_given || !levels_out_file.empty() || !levels_in_file.empty()) ? "the levels of one image ('--tile-dither', '--tile-levels-out', '--tile-levels-in')" : nullptr);
        if (bad) { fprintf(stderr, "error: the argument '%s' cannot be used with %s\n", opt, bad); return 2; }
        if (shares.empty()) { fprintf(stderr, "error: '%s' needs '--share <SOURCE=TARGET>': it chooses the dither levels of a set (one image: --tile-dither)\n", opt); return 2; }
        if (!ordered_given) { fprintf(stderr, "error: '%s' needs '--ordered-dither <N>'\n", opt); return 2; }
        char *end = nullptr;
        if (set_level_given) {
            const unsigned long k = strtoul(set_level_arg.c_str(), &end, 10);
            if (set_level_arg.empty() || set_level_arg[0] == '-' || *end || k < 1 || k > 1000000) { fprintf(stderr, "error: invalid value '%s' for '--set-tile-dither <K>': expected a number of sweeps, 1 or more\n", set_level_arg.c_str()); return 2; }
            set_level_every = (uint32_t)k;
        }
        if (set_mode_given) {
            if (set_mode_arg != "tied" && set_mode_arg != "frame") { fprintf(stderr, "error: invalid value '%s' for '--set-levels <tied|frame>': expected tied or frame\n", set_mode_arg.c_str()); return 2; }
            set_tied = set_mode_arg == "tied";
        }
        if (dither_levels_given) {
            const unsigned long l = strtoul(dither_levels_arg.c_str(), &end, 10);
            if (dither_levels_arg.empty() || *end || l < 2 || l > 8) { fprintf(stderr, "error: invalid value '%s' for '--dither-levels <L>': expected 2..8\n", dither_levels_arg.c_str()); return 2; }
            dither_levels = (uint32_t)l;
        }
        if (!set_level_given && set_levels_in_file.empty()) { fprintf(stderr, "error: '%s' needs '--set-tile-dither <K>' or '--set-tile-levels-in <F>'\n", opt); return 2; }
        if (set_levels_in_file.empty() && ordered_amp < dither_levels - 1) {
            fprintf(stderr, "error: '--dither-levels %u' needs '--dither-amplitude' of at least %u: every level is a different amplitude\n", dither_levels, dither_levels - 1); return 2; }
        if (!set_levels_in_file.empty()) {
            const std::string &file = set_levels_in_file;
            long n_in = 0; bool tied_in = false;
            if (!json_int_scalar(file, "n", n_in) || !json_int_array(file, "amplitudes", level_amps) || !json_bool(file, "tied", tied_in) || !json_int_arrays(file, "frames", set_levels_in))
                die("cannot read n, amplitudes, tied and frames from " + file);
            if (n_in != (long)ordered_n) die(file + " was written for --ordered-dither " + std::to_string(n_in));
            if (level_amps.empty() || level_amps.size() > 8) die(file + ": 1 to 8 amplitudes expected");
            for (long a : level_amps) if (a < 0 || a > 255) die(file + ": amplitude out of range");
            if (set_levels_in.size() != shares.size() + 1) die(file + " holds the levels of " + std::to_string(set_levels_in.size()) + " frames, the set has " + std::to_string(shares.size() + 1));
            bool differ = false;
            for (const auto &fr : set_levels_in) {
                for (long l : fr) if (l < 0 || l >= (long)level_amps.size()) die(file + ": level out of range");
                differ = differ || fr != set_levels_in[0];
            }
            if (tied_in && differ) die(file + " says tied, but its frames differ in level");
            if (set_tied && differ) die(file + ": the frames differ in level, which --set-levels tied does not take (name --set-levels frame)");
            // the ladder is the file's: a --dither-levels or --dither-amplitude that says otherwise is a mistake, not a preference
            if (dither_levels_given && dither_levels != level_amps.size()) die(file + " holds " + std::to_string(level_amps.size()) + " levels, --dither-levels says " + std::to_string(dither_levels));
            const long top = *std::max_element(level_amps.begin(), level_amps.end());
            if (amp_given && (long)ordered_amp != top) die(file + " was written for --dither-amplitude " + std::to_string(top) + ", the command line says " + std::to_string(ordered_amp));
            ordered_amp = (uint32_t)top; // (what the log reports)
        } else for (uint32_t j = 0; j < dither_levels; j++) level_amps.push_back((long)(ordered_amp * j / (dither_levels - 1)));
    }
    std::vector<int8_t> level_bank(256 * level_amps.size(), 0); // table j at n*n*j: zeros for amplitude 0
    for (size_t j = 0; j < level_amps.size(); j++) if (level_amps[j]) snesimage_bayer_offsets(ordered_n, (uint32_t)level_amps[j], &level_bank[(size_t)ordered_n * ordered_n * j]);
    // every context of the run gets the table before anything is computed on it (the initialisers end with optimize(), which sees it)
    auto create = [&](const uint8_t *px, uint32_t cw, uint32_t chh, int dev, snesimage_ctx **out) -> int32_t {
        int32_t rc = snesimage_create(px, cw, chh, count, size, flags, dev, out);
        if (rc == 0 && !level_amps.empty() && !set_level_opts) rc = snesimage_set_ordered_dither_bank(*out, level_bank.data(), ordered_n, (uint32_t)level_amps.size(), (uint32_t)level_amps.size() - 1); // (tiles start on the full amplitude)
        else if (rc == 0 && ordered_n) rc = snesimage_set_ordered_dither(*out, ordered_tab, ordered_n);
        return rc;
    };
    if (backdrop || backdrop_fixed) { // said before any device is touched
        const char *opt = backdrop_fixed ? "--backdrop-fixed" : "--backdrop";
        if (backdrop_fixed) {
            unsigned v[3]; char tail = 0;
            if (sscanf(backdrop_arg.c_str(), "%u,%u,%u%c", &v[0], &v[1], &v[2], &tail) != 3 || v[0] > 31 || v[1] > 31 || v[2] > 31) {
                fprintf(stderr, "error: invalid value '%s' for '--backdrop-fixed <R,G,B>': expected three 5-bit values, such as 0,0,31\n", backdrop_arg.c_str()); return 1; }
            for (int k = 0; k < 3; k++) backdrop_rgb[k] = (uint8_t)v[k];
        }
        if (!shares.empty() || !devices.empty()) { fprintf(stderr, "error: '%s' cannot be used with '%s': sets and device groups do not carry the backdrop colour yet\n", opt, !shares.empty() ? "--share" : "--devices"); return 1; }
        if (size > 15 || (unsigned long long)count * (size + 1) > 253) {
            fprintf(stderr, "error: '%s' needs --subpalette-size <= 15 and count * (size + 1) <= 253: a row of 16 colours holds the backdrop colour and 15 of its own\n", opt); return 1; }
        flags |= SNES_BACKDROP;
    }
    const bool bd_fixed = backdrop_fixed || set_backdrop_fixed;
    const bool bd = (flags & SNES_BACKDROP) != 0, bd_sched = bd && !bd_fixed; // --backdrop-fixed and --set-backdrop-fixed run the plain schedule: B is never a call's slot
    auto sched_next = [&](uint32_t *p, uint32_t *ix, uint32_t *ch, uint32_t *st, uint32_t *m) {
        if (bd_sched) snesimage_schedule_next_backdrop(count, size, (flags & SNES_NES) ? 1 : 0, p, ix, ch, st, m); else snesimage_schedule_next(count, size, (flags & SNES_NES) ? 1 : 0, p, ix, ch, st, m);
    };
    // the JSON keeps 15 colours per subpalette (src/lib.rs:583-593): a larger subpalette cannot be read back from it
    if (!resume_file.empty() && size > 15) die("--resume needs --subpalette-size <= 15: the output keeps 15 colours per subpalette");

    log_info("Using source image: " + source); // src/lib.rs:834
    std::vector<uint8_t> rgba;
    uint32_t w = 256, h = 256;
    load_source(source, w, h, rgba);
    if (blocks_given && (h / 8) % blocks_h) { // known once the image is decoded: said before any device is touched
        fprintf(stderr, "error: invalid value '%s' for '--palette-blocks <WxH>': H must divide the image's %u rows of tiles\n", blocks_arg.c_str(), h / 8); return 2; }
    if (decode_only) {
        FILE *f = fopen(target.c_str(), "wb");
        if (!f) die("cannot create " + target);
        fwrite(rgba.data(), 1, rgba.size(), f);
        fclose(f);
        printf("%u %u\n", w, h);
        return 0;
    }
    std::vector<std::vector<uint8_t>> shared_rgba(shares.size()); // every --share source, decoded like the main one
    for (size_t i = 0; i < shares.size(); i++) {
        uint32_t ow = 0, oh = 0;
        log_info("Using shared image: " + shares[i].first);
        load_source(shares[i].first, ow, oh, shared_rgba[i]);
        if (ow != w || oh != h) die("shared image " + shares[i].first + " is " + std::to_string(ow) + "x" + std::to_string(oh) + ", the source " + std::to_string(w) + "x" + std::to_string(h));
    }
    if ((max_set_given || !set_tilemap_file.empty()) && (uint64_t)(shares.size() + 1) * (w / 8) * (h / 8) > 8192) // known once the images are decoded: said before the run, not after it
        die(std::string(max_set_given ? "--max-set-tiles" : "--set-tilemap") + ": the set has " + std::to_string((uint64_t)(shares.size() + 1) * (w / 8) * (h / 8)) +
            " tiles in all; the character budget of a set takes at most 8192 (eight frames of 256 x 256, nine of 256 x 224)");
    // the native files of an import, read and sized before a device is touched: CGRAM 512 bytes, one tilemap word per tile (of every
    // frame), whole characters of the depth named or implied
    std::vector<uint8_t> in_cgram, in_chr, in_map;
    const bool importing = import_first >= 0 || set_import_first >= 0;
    if (importing) {
        const bool of_set = set_import_first >= 0;
        const std::string *files = of_set ? set_import_file : import_file;
        std::vector<uint8_t> *into[3] = {&in_cgram, &in_chr, &in_map};
        for (int k = 0; k < 3; k++) {
            FILE *f = fopen(files[k].c_str(), "rb");
            if (!f) { fprintf(stderr, "error: cannot read '%s'\n", files[k].c_str()); return 2; }
            uint8_t buf[65536]; size_t n;
            while ((n = fread(buf, 1, sizeof buf, f)) > 0 && into[k]->size() <= (1u << 20)) into[k]->insert(into[k]->end(), buf, buf + n);
            fclose(f);
        }
        const size_t words = 32 * (size_t)(h / 8) * (of_set ? shares.size() + 1 : 1);
        const unsigned long bpp = import_opt[0].value ? import_opt[0].value : (size <= 3 ? 2 : (size <= 15 ? 4 : 8));
        if (in_cgram.size() != 512) { fprintf(stderr, "error: '%s' holds %zu bytes: a CGRAM image is 512\n", files[0].c_str(), in_cgram.size()); return 2; }
        if (in_map.size() != 2 * words) { fprintf(stderr, "error: '%s' holds %zu bytes: %zu tilemap words of 2 bytes are expected\n", files[2].c_str(), in_map.size(), words); return 2; }
        if (in_chr.empty() || in_chr.size() % (8 * bpp) || in_chr.size() / (8 * bpp) > 1024) {
            fprintf(stderr, "error: '%s' holds %zu bytes: 1 to 1024 whole characters of %lu bytes (%lubpp) are expected\n", files[1].c_str(), in_chr.size(), 8 * bpp, bpp); return 2; }
    }
    snesimage_native_layout in_lay{};
    in_lay.bpp = (uint8_t)import_opt[0].value; in_lay.char_base = (uint16_t)import_opt[1].value; in_lay.palette_base = (uint8_t)import_opt[2].value;
    auto log_import = [&](const snesimage_native_info &ni, const char *of) {
        log_info(std::string("Imported native data") + of + ": " + std::to_string(ni.bpp) + "bpp, " + std::to_string(ni.unique) + " characters at " + std::to_string(in_lay.char_base) + ", " +
                 std::to_string(ni.map_words) + " tilemap words");
    };
    if (!devices.empty()) device = devices[0];
    snesimage_ctx *ctx = nullptr;
    if (create(rgba.data(), w, h, device, &ctx) != 0) die(snesimage_last_error());
    if (gd.proxy != SNES_GUIDE_REDMEAN && snesimage_set_guided_proxy(ctx, gd.proxy) != 0) die(snesimage_last_error()); // (before the context is lent to anything)
    if (blocks_given) { // before the initialisers, --resume and --tile-palettes: they cluster, and are held to, the blocks
        if (snesimage_set_palette_blocks(ctx, blocks_w, blocks_h) != 0) die(snesimage_last_error());
        log_info("Palette blocks: one subpalette per " + std::to_string(blocks_w) + " x " + std::to_string(blocks_h) + " tiles");
    }
    if (ordered_n) log_info("Ordered dithering: " + std::to_string(ordered_n) + " x " + std::to_string(ordered_n) + " Bayer pattern, amplitude " + std::to_string(ordered_amp));
    if (!level_amps.empty() && !set_level_opts) {
        std::string m = "Per-tile dither levels: " + std::to_string(level_amps.size()) + " levels, amplitudes";
        for (size_t j = 0; j < level_amps.size(); j++) m += (j ? ", " : " ") + std::to_string(level_amps[j]);
        log_info(m);
        if (!levels_in_file.empty()) {
            if (levels_in.size() != 32 * (size_t)(h / 8)) die(levels_in_file + " does not match the image: one level per 8 x 8 tile expected (" + std::to_string(32 * (size_t)(h / 8)) + ")");
            std::vector<uint8_t> lv(1024, 0);
            for (size_t i = 0; i < levels_in.size(); i++) lv[i] = (uint8_t)levels_in[i];
            if (snesimage_set_tile_levels(ctx, lv.data()) != 0) die(snesimage_last_error());
            log_info("Tile levels from " + levels_in_file);
        }
    }
    if (backdrop_fixed && snesimage_set_backdrop_rgb5(ctx, backdrop_rgb) != 0) die(snesimage_last_error()); // (the initialisers end with optimize(), which sees it)
    // palette + tile_palettes (+ B, from slot 0) of an earlier output (src/lib.rs:579-625); the tiles follow from optimize()
    auto read_resume = [&](const std::string &file, std::vector<uint8_t> &tp8, std::vector<uint8_t> &rgb5, uint8_t *b) {
        std::vector<long> pal, tp;
        if (!json_int_array(file, "palette", pal) || !json_int_array(file, "tile_palettes", tp)) die("cannot read palette and tile_palettes from " + file);
        // as_json writes one tile palette per tile of the image (src/lib.rs:598-616): 32 per 8 rows, 1,024 at 256 rows, 896 at 224
        const size_t ntiles = 32 * (size_t)(h / 8);
        if (pal.size() != 16 * (size_t)count || tp.size() != ntiles)
            die("resume file does not match the image and --subpalette-count (palette must hold 16 entries per subpalette, tile_palettes one per 8 x 8 tile: " + std::to_string(ntiles) + ")");
        tp8.assign(1024, 0); rgb5.assign(3 * (size_t)count * size, 0); // (the rows of tiles below the image keep subpalette 0, as after snesimage_create)
        for (size_t i = 0; i < ntiles; i++) { if (tp[i] < 0 || tp[i] >= (long)count) die("resume file: tile palette out of range"); tp8[i] = (uint8_t)tp[i]; }
        for (uint32_t p = 0; p < count; p++)
            for (uint32_t i = 0; i < size; i++) { // slot 0 of every 16 is the transparent colour (src/lib.rs:583-585)
                const long v = pal[16 * (size_t)p + 1 + i];
                if (v < 0 || v > 0x7fff) die("resume file: colour out of range");
                uint8_t *o = &rgb5[3 * ((size_t)p * size + i)];
                o[0] = (uint8_t)(v & 31); o[1] = (uint8_t)((v >> 5) & 31); o[2] = (uint8_t)((v >> 10) & 31);
            }
        const long v = pal[0]; // a backdrop run wrote B into slot 0 of every row (and 0 into `tiles` where a pixel shows it: optimize() finds those again)
        if (bd && (v < 0 || v > 0x7fff)) die("resume file: colour out of range");
        b[0] = (uint8_t)(v & 31); b[1] = (uint8_t)((v >> 5) & 31); b[2] = (uint8_t)((v >> 10) & 31);
    };
    // --share: one context per image, every member's storage sized for one call's candidates (about 4.45 MB each), one set
    std::vector<snesimage_ctx *> frames{ctx};
    snesimage_shared *set = nullptr;
    if (!shares.empty()) {
        for (const auto &other : shared_rgba) {
            snesimage_ctx *m = nullptr;
            if (create(other.data(), w, h, device, &m) != 0) die(snesimage_last_error());
            frames.push_back(m);
        }
        uint32_t chunk = ncand > 32 ? ncand : 32; // the largest call of the schedule: random (ncand), channel (32) or NES (56)
        if ((flags & SNES_NES) && chunk < 56) chunk = 56;
        for (snesimage_ctx *m : frames) if (snesimage_set_chunk(m, chunk) != 0) die(snesimage_last_error());
        const uint8_t *set_b = set_backdrop_fixed ? backdrop_rgb : nullptr; // nullptr: the mean of all frames' opaque pixels
        uint8_t resumed_b[3] = {0, 0, 0};
        if (set_bd && !resume_file.empty()) { // every frame from its own earlier output: the main one from --resume, the others from their targets
            for (size_t i = 0; i < frames.size(); i++) {
                const std::string &file = i ? shares[i - 1].second : resume_file;
                std::vector<uint8_t> tp8, rgb5; uint8_t b[3];
                read_resume(file, tp8, rgb5, b);
                if (i == 0) memcpy(resumed_b, b, 3);
                if (snesimage_set_tile_palettes(frames[i], tp8.data()) != 0 || snesimage_set_palette_rgb5(frames[i], rgb5.data()) != 0) die(snesimage_last_error());
            }
            if (!set_backdrop_fixed) set_b = resumed_b;
        }
        if ((set_bd ? snesimage_shared_create_backdrop(frames.data(), (uint32_t)frames.size(), set_b, &set) : snesimage_shared_create(frames.data(), (uint32_t)frames.size(), &set)) != 0) die(snesimage_last_error());
        log_info("Sharing one palette between " + std::to_string(frames.size()) + " images");
        if (sgd.proxy != SNES_GUIDE_REDMEAN && snesimage_shared_set_guided_proxy(set, sgd.proxy) != 0) die(snesimage_last_error());
        if (set_bd) {
            uint8_t b[3];
            if (snesimage_shared_get_backdrop_rgb5(set, b) != 0) die(snesimage_last_error());
            char m[120];
            snprintf(m, sizeof m, "Backdrop colour of the set%s: (%u, %u, %u)", set_backdrop_fixed ? " (fixed)" : "", b[0], b[1], b[2]);
            log_info(m);
            if (!resume_file.empty()) log_info("Resumed the set from " + resume_file + " and the --share targets");
        }
        if (set_level_opts) { // the set owns the bank; every tile of every frame starts on the full amplitude, the table the frames were created with
            const uint32_t L = (uint32_t)level_amps.size();
            if (snesimage_shared_set_ordered_dither_bank(set, level_bank.data(), ordered_n, L, L - 1) != 0) die(snesimage_last_error());
            std::string m = std::string("Per-tile dither levels of the set (") + (set_tied ? "tied" : "per frame") + "): " + std::to_string(L) + " levels, amplitudes";
            for (size_t j = 0; j < level_amps.size(); j++) m += (j ? ", " : " ") + std::to_string(level_amps[j]);
            log_info(m);
            if (!set_levels_in_file.empty()) {
                for (size_t i = 0; i < frames.size(); i++) {
                    if (set_levels_in[i].size() != 32 * (size_t)(h / 8)) die(set_levels_in_file + " does not match the images: one level per 8 x 8 tile expected (" + std::to_string(32 * (size_t)(h / 8)) + ")");
                    std::vector<uint8_t> lv(1024, 0);
                    for (size_t t = 0; t < set_levels_in[i].size(); t++) lv[t] = (uint8_t)set_levels_in[i][t];
                    if (snesimage_shared_set_tile_levels(set, (uint32_t)i, lv.data()) != 0) die(snesimage_last_error());
                }
                log_info("Tile levels of the set from " + set_levels_in_file);
            }
        }
    }
    if (!resume_file.empty()) {
        if (!set) { // (a backdrop set was resumed above, before it was formed)
            std::vector<uint8_t> tp8, rgb5; uint8_t b[3];
            read_resume(resume_file, tp8, rgb5, b);
            if (bd && !backdrop_fixed && snesimage_set_backdrop_rgb5(ctx, b) != 0) die(snesimage_last_error());
            if (snesimage_set_tile_palettes(ctx, tp8.data()) != 0 || snesimage_set_palette_rgb5(ctx, rgb5.data()) != 0 || snesimage_optimize(ctx) != 0) die(snesimage_last_error());
            log_info("Resumed from " + resume_file);
        }
    } else if (importing) { // the state is the files': no initialiser runs, and the map is a stored map until an optimizer call replaces it
        snesimage_native_info ni{};
        const uint16_t *words = reinterpret_cast<const uint16_t *>(in_map.data()); // (the words are little-endian as the host is)
        if ((set ? snesimage_shared_import_native(set, &in_lay, in_cgram.data(), in_chr.data(), in_chr.size(), words, &ni)
                 : snesimage_import_native(ctx, &in_lay, in_cgram.data(), in_chr.data(), in_chr.size(), words, &ni)) != 0) die(std::string("Unable to import native data: ") + snesimage_last_error());
        log_import(ni, set ? " of the set" : "");
    } else if (set) { // the reference's initialisers on the images stacked top to bottom
        if (snesimage_shared_initialize_tiles(set) != 0) die(std::string("Unable to initialize tiles: ") + snesimage_last_error());
        log_info("Finished assigning initial tiles");
        log_info("Generating initial palettes");
        if (snesimage_shared_recalculate_palettes(set) != 0) die(std::string("Unable to recalculate palettes: ") + snesimage_last_error());
    } else {
        if (snesimage_initialize_tiles(ctx) != 0) die(std::string("Unable to initialize tiles: ") + snesimage_last_error()); // src/lib.rs:851-853
        log_info("Finished assigning initial tiles");
        if (!tile_file.empty()) {
            std::vector<uint8_t> tp(1024);
            FILE *f = fopen(tile_file.c_str(), "rb");
            if (!f || fread(tp.data(), 1, 1024, f) != 1024) die("cannot read 1024 bytes from " + tile_file);
            fclose(f);
            if (snesimage_set_tile_palettes(ctx, tp.data()) != 0) die(snesimage_last_error());
        }
        log_info("Generating initial palettes"); // src/lib.rs:985-989
        if (snesimage_recalculate_palettes(ctx) != 0) die(std::string("Unable to recalculate palettes: ") + snesimage_last_error());
    }
    // --devices: replicas of the initialised state on the other devices, and the group that shards each call over them
    std::vector<snesimage_ctx *> members{ctx};
    snesimage_group *group = nullptr;
    if (!devices.empty()) {
        std::vector<uint8_t> tp(1024), pal(3 * (size_t)count * size);
        if (snesimage_get_tile_palettes(ctx, tp.data()) != 0 || snesimage_get_palette_rgb5(ctx, pal.data()) != 0) die(snesimage_last_error());
        for (size_t d = 1; d < devices.size(); d++) {
            snesimage_ctx *m = nullptr;
            if (create(rgba.data(), w, h, devices[d], &m) != 0 || snesimage_set_tile_palettes(m, tp.data()) != 0 || snesimage_set_palette_rgb5(m, pal.data()) != 0 ||
                snesimage_optimize(m) != 0)
                die(snesimage_last_error());
            members.push_back(m);
        }
        if (snesimage_group_create(members.data(), (uint32_t)members.size(), &group) != 0) die(snesimage_last_error());
        log_info("Sharding candidates over " + std::to_string(members.size()) + " device(s)"); // (with the reference's 64 candidates per call: the calls of every window)
    }
    log_info("Beginning optimization"); // src/lib.rs:992
    uint32_t palette = 0, index = 0, channel = 0, step = 0, sweep = 0;
    double last_error = 1.7976931348623157e308;
    std::vector<uint8_t> before(3 * ((size_t)count * size + 1)), after(before.size()); // (+ the backdrop colour, behind the last entry: slot (count, 0))
    auto load_before = [&]() { if (snesimage_get_palette_rgb5(ctx, before.data()) != 0 || (bd && snesimage_get_backdrop_rgb5(ctx, &before[3 * (size_t)count * size]) != 0)) die(snesimage_last_error()); };
    auto report = [&](uint32_t p, uint32_t ix, const uint8_t *b, const uint8_t *best, double error) {
        if (b[0] != best[0] || b[1] != best[1] || b[2] != best[2]) { // src/lib.rs:222-234
            char m[160];
            snprintf(m, sizeof m, "Setting color (%u, %u) from (%u, %u, %u) to (%u, %u, %u)", p, ix, b[0], b[1], b[2], best[0], best[1], best[2]);
            log_info(m);
        }
        if (std::abs(error - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(error)); last_error = error; } // src/lib.rs:912-915
    };
    auto level_sweep = [&]() { // one level sweep over the whole image, each call decided by error()
        snesimage_run_stats ts{};
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_error(ctx, &e0) != 0 || snesimage_level_sweep(ctx, 0, 32 * (h / 8), 0, nullptr, &ts) != 0 || snesimage_error(ctx, &e1) != 0) die(std::string("Unable to choose dither levels: ") + snesimage_last_error());
        log_info("Tile dither: " + std::to_string(ts.calls) + " calls, " + std::to_string(ts.accepted) + " accepted in " + std::to_string(ts.windows) + " launch sets; error " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (std::abs(e1 - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(e1)); last_error = e1; }
    };
    auto set_level_sweep = [&]() { // one level sweep of the set over all tiles: tied calls decided by E, or every frame's own calls
        snesimage_run_stats ts{};
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_shared_error(set, &e0) != 0 || snesimage_shared_level_sweep(set, 0, 32 * (h / 8), 0, set_tied ? 1 : 0, nullptr, &ts) != 0 || snesimage_shared_error(set, &e1) != 0)
            die(std::string("Unable to choose the dither levels of the set: ") + snesimage_last_error());
        log_info(std::string("Set tile dither (") + (set_tied ? "tied" : "per frame") + "): " + std::to_string(ts.calls) + " calls, " + std::to_string(ts.accepted) + " accepted in " + std::to_string(ts.windows) +
                 " launch sets; error " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (std::abs(e1 - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(e1)); last_error = e1; }
    };
    auto guided_sweep = [&]() { // one guided call on every slot, each decided by error(); --backdrop-fixed passes the backdrop slot by
        snesimage_run_stats gs{};
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_error(ctx, &e0) != 0) die(std::string("Unable to run a guided sweep: ") + snesimage_last_error());
        // through the slot windows, --window calls per launch set (1: call by call; the same result); count * size calls from (0, 0) end in front of the backdrop slot
        uint32_t gp = 0, gi = 0;
        if (snesimage_guided_run_slots(ctx, count * size + (bd_sched ? 1u : 0u), gd.shortlist, &gp, &gi, window, nullptr, &gs) != 0) die(std::string("Unable to run a guided sweep: ") + snesimage_last_error());
        if (snesimage_error(ctx, &e1) != 0) die(std::string("Unable to run a guided sweep: ") + snesimage_last_error());
        log_info("Guided sweep: " + std::to_string(gs.calls) + " calls, " + std::to_string(gs.accepted) + " accepted (" + gd.proxy_name() + "); error " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (std::abs(e1 - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(e1)); last_error = e1; }
        load_before(); // (the colours the next calls' reports compare with)
    };
    auto set_guided_sweep = [&]() { // one guided call of the set on every slot, each decided by E; --set-backdrop-fixed passes the backdrop slot by
        const std::string what = "Unable to run a guided sweep of the set: ";
        snesimage_run_stats gs{};
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_shared_error(set, &e0) != 0) die(what + snesimage_last_error());
        // through the set's slot windows, --window calls per launch set (1: call by call; the same result); count * size calls from (0, 0) end in front of the backdrop slot
        uint32_t gp = 0, gi = 0;
        if (snesimage_shared_guided_run_slots(set, count * size + (set_bd && !bd_fixed ? 1u : 0u), sgd.shortlist, &gp, &gi, window, nullptr, &gs) != 0) die(what + snesimage_last_error());
        if (snesimage_shared_error(set, &e1) != 0) die(what + snesimage_last_error());
        log_info("Guided sweep of the set: " + std::to_string(gs.calls) + " calls, " + std::to_string(gs.accepted) + " accepted (" + sgd.proxy_name() + "); error " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (std::abs(e1 - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(e1)); last_error = e1; }
        load_before(); // (the colours the next calls' reports compare with)
    };
    auto end_of_sweep = [&]() {
        if (gd.every && step != sweep && step % gd.every == 0) guided_sweep(); // in front of everything that moves tiles: they see the palette it leaves
        if (sgd.every && step != sweep && step % sgd.every == 0) set_guided_sweep(); // (the same place for a set)
        if (reassign_every && step != sweep && step % reassign_every == 0) { // a sweep over every slot has just ended (src/lib.rs:925-931)
            uint32_t moved = 0;
            if (set) { if (snesimage_shared_reassign_tiles(set, &moved) != 0) die(std::string("Unable to reassign tiles: ") + snesimage_last_error()); }
            else for (snesimage_ctx *m : members) if (snesimage_reassign_tiles(m, &moved) != 0) die(std::string("Unable to reassign tiles: ") + snesimage_last_error());
            log_info("Reassigned " + std::to_string(moved) + " tiles");
        }
        if (tile_every && step != sweep && step % tile_every == 0) { // one tile sweep over the whole image, each call decided by error()
            const uint32_t ntile = 32 * (h / 8), nblock = (32 / blocks_w) * ((h / 8) / blocks_h);
            snesimage_run_stats ts{};
            double e = 0.0;
            if (set          ? (snesimage_shared_tile_sweep(set, 0, ntile, 0, nullptr, &ts) != 0 || snesimage_shared_error(set, &e) != 0)
                : blocks_given ? (snesimage_block_sweep(ctx, 0, nblock, 0, nullptr, &ts) != 0 || snesimage_error(ctx, &e) != 0) // a block sweep over all blocks
                               : (snesimage_tile_sweep(ctx, 0, ntile, 0, nullptr, &ts) != 0 || snesimage_error(ctx, &e) != 0)) die(std::string("Unable to move tiles: ") + snesimage_last_error());
            log_info("Moved " + std::to_string(ts.accepted) + (blocks_given ? " blocks in " : " tiles in ") + std::to_string(ts.windows) + " launch sets");
            if (std::abs(e - last_error) > 2.220446049250313e-16) { log_info("Current Error: " + fmt_f64(e)); last_error = e; }
        }
        if (level_every && step != sweep && step % level_every == 0) level_sweep(); // behind the tile moves: the levels are chosen for the subpalettes the tiles ended on
        if (set_level_every && step != sweep && step % set_level_every == 0) set_level_sweep();
        sweep = step;
    };
    if (ncand <= 64 && window != 1) {
        // The reference's loop (src/lib.rs:888-933), several calls per launch: snesimage_run_slots scores the coming calls of the
        // schedule against the current palette and applies them in order up to the first one that changes it — the same
        // trajectory, call for call, as stepping one call at a time (--window 1).  A run ends with its sweep when tiles are
        // to be reassigned between sweeps.  --share: snesimage_shared_run_slots, the same for a set (the records carry E).
        std::vector<snesimage_call_result> log;
        load_before();
        snesimage_run_stats total{};
        for (uint32_t call = 0; call < calls;) {
            uint32_t n = calls - call;
            if (n > 4096) n = 4096;
            if (reassign_every || tile_every || level_every || set_level_every || gd.every || sgd.every || bd_fixed) { // calls left in the current sweep
                uint32_t p = palette, ix = index, ch = channel, st = step, m = 0, k = 0;
                while (st == step && k < n) { sched_next(&p, &ix, &ch, &st, &m); k++; }
                n = k;
            }
            log.resize(n);
            uint32_t p = palette, ix = index, ch = channel, st = step, method = 0;
            snesimage_run_stats rs{};
            if ((set   ? snesimage_shared_run_slots(set, n, seed, call, &palette, &index, &channel, &step, ncand, window, log.data(), &rs)
                 : group ? snesimage_group_run_slots(group, n, seed, call, &palette, &index, &channel, &step, ncand, window, log.data(), &rs)
                         : snesimage_run_slots(ctx, n, seed, call, &palette, &index, &channel, &step, ncand, window, log.data(), &rs)) != 0) die(std::string("Unable to optimize palette: ") + snesimage_last_error());
            total.calls += rs.calls; total.accepted += rs.accepted; total.windows += rs.windows; total.scored += rs.scored; total.useful += rs.useful;
            if (bd_fixed && palette == count) { palette = 0; index = 0; channel = 0; step += 1; } // the library's schedule has arrived at the backdrop slot: this run passes it by
            for (uint32_t j = 0; j < n; j++) {
                const uint32_t cp = p, ci = ix;
                sched_next(&p, &ix, &ch, &st, &method);
                uint8_t *b = &before[3 * ((size_t)cp * size + ci)];
                report(cp, ci, b, log[j].rgb5, log[j].error);
                b[0] = log[j].rgb5[0]; b[1] = log[j].rgb5[1]; b[2] = log[j].rgb5[2];
            }
            call += n;
            end_of_sweep();
        }
        if (calls) {
            char m[200];
            snprintf(m, sizeof m, "Ran %u calls in %u launch sets: %u changed the palette, %llu of %llu candidates scored were of calls that took effect", total.calls, total.windows, total.accepted,
                     (unsigned long long)total.useful, (unsigned long long)total.scored);
            log_info(m);
        }
    } else
    for (uint32_t call = 0; call < calls; call++) {
        uint32_t p = palette, ix = index, ch = channel, method = 0;
        sched_next(&palette, &index, &channel, &step, &method);
        load_before();
        double error = 0.0; uint8_t best[3];
        const int32_t rc = set ? snesimage_shared_step(set, method, p, ix, ch, seed, call, method == SNES_METHOD_RANDOM ? ncand : 0, &error, best)
                         : group ? snesimage_group_step(group, method, p, ix, ch, seed, call, method == SNES_METHOD_RANDOM ? ncand : 0, &error, best)
                                 : snesimage_step(ctx, method, p, ix, ch, seed, call, method == SNES_METHOD_RANDOM ? ncand : 0, &error, best);
        if (rc != 0) die(std::string("Unable to optimize palette: ") + snesimage_last_error());
        report(p, ix, &before[3 * ((size_t)p * size + ix)], best, error);
        end_of_sweep();
    }
    if (level_every) level_sweep(); // once behind the last call; the character budget and the refit run behind it
    if (set_level_every) set_level_sweep(); // in front of --max-set-tiles and --refit-set-tiles
    if (max_tiles_given) { // the last stage: anything that re-runs optimize() would replace the merged map
        uint32_t u0 = 0, u1 = 0, merges = 0;
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_characters(ctx, &u0, nullptr, nullptr, nullptr) != 0 || snesimage_error(ctx, &e0) != 0) die(std::string("Unable to count characters: ") + snesimage_last_error());
        if (snesimage_reduce_characters(ctx, max_tiles, merge_short, nullptr, 0, &merges, &u1) != 0 || snesimage_error(ctx, &e1) != 0) die(std::string("Unable to merge tiles: ") + snesimage_last_error());
        log_info("Characters: " + std::to_string(u0) + " -> " + std::to_string(u1) + " in " + std::to_string(merges) + " merges (budget " + std::to_string(max_tiles) + ")");
        log_info("Error: " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (u1 > max_tiles) log_info("No tile is left that may be merged: the budget is not met");
    }
    for (uint32_t sweep = 0; sweep < refit_sweeps; sweep++) { // behind the merges, in front of everything that is written: a refit is the last stage too
        uint32_t n_calls = 0, n_acc = 0, u1 = 0;
        double e0 = 0.0, e1 = 0.0;
        snesimage_run_stats rs{};
        if (snesimage_error(ctx, &e0) != 0 || snesimage_refit_characters(ctx, 0, nullptr, 0, &n_calls, &n_acc, &u1, &rs) != 0 || snesimage_error(ctx, &e1) != 0)
            die(std::string("Unable to refit characters: ") + snesimage_last_error());
        const uint32_t skipped = n_calls - (uint32_t)rs.useful;
        log_info("Refit sweep " + std::to_string(sweep + 1) + ": " + std::to_string(n_calls) + " calls, " + std::to_string(n_acc) + " accepted, " + std::to_string(skipped) + " skipped; error " +
                 fmt_f64(e0) + " -> " + fmt_f64(e1) + "; " + std::to_string(u1) + " characters");
        if (n_acc == 0) break;
    }
    if (max_set_given) { // the set's budget, behind the last optimizer call and in front of everything that is written
        uint32_t u0 = 0, u1 = 0, merges = 0;
        double e0 = 0.0, e1 = 0.0;
        if (snesimage_shared_characters(set, &u0, nullptr, nullptr, nullptr) != 0 || snesimage_shared_error(set, &e0) != 0) die(std::string("Unable to count characters: ") + snesimage_last_error());
        if (snesimage_shared_reduce_characters(set, max_set_tiles, merge_short, nullptr, 0, &merges, &u1) != 0 || snesimage_shared_error(set, &e1) != 0)
            die(std::string("Unable to merge tiles: ") + snesimage_last_error());
        log_info("Characters of the set: " + std::to_string(u0) + " -> " + std::to_string(u1) + " in " + std::to_string(merges) + " merges (budget " + std::to_string(max_set_tiles) + ")");
        log_info("Error: " + fmt_f64(e0) + " -> " + fmt_f64(e1));
        if (u1 > max_set_tiles) log_info("No tile is left that may be merged: the budget is not met");
    }
    for (uint32_t sweep = 0; sweep < refit_set_sweeps; sweep++) { // behind the set's merges, in front of everything that is written: a refit is the last stage too
        uint32_t n_calls = 0, n_acc = 0, u1 = 0;
        double e0 = 0.0, e1 = 0.0;
        snesimage_run_stats rs{};
        if (snesimage_shared_error(set, &e0) != 0 || snesimage_shared_refit_characters(set, 0, nullptr, 0, &n_calls, &n_acc, &u1, &rs) != 0 || snesimage_shared_error(set, &e1) != 0)
            die(std::string("Unable to refit the characters of the set: ") + snesimage_last_error());
        const uint32_t skipped = n_calls - (uint32_t)rs.useful;
        log_info("Refit sweep of the set " + std::to_string(sweep + 1) + ": " + std::to_string(n_calls) + " calls, " + std::to_string(n_acc) + " accepted, " + std::to_string(skipped) +
                 " skipped; error " + fmt_f64(e0) + " -> " + fmt_f64(e1) + "; " + std::to_string(u1) + " characters");
        if (n_acc == 0) break;
    }
    log_info("Writing output to " + target); // src/lib.rs:1000-1002
    write_json(ctx, target);
    for (size_t i = 0; i < shares.size(); i++) {
        log_info("Writing output to " + shares[i].second);
        write_json(frames[i + 1], shares[i].second);
    }
    if (!levels_out_file.empty()) { // what the main JSON does not record: the ladder and every tile's level
        std::vector<uint8_t> lv(1024);
        if (snesimage_get_tile_levels(ctx, lv.data()) != 0) die(snesimage_last_error());
        std::string js = "{\"n\":" + std::to_string(ordered_n) + ",\"amplitudes\":[";
        for (size_t j = 0; j < level_amps.size(); j++) js += (j ? "," : "") + std::to_string(level_amps[j]);
        js += "],\"levels\":[";
        for (size_t i = 0; i < 32 * (size_t)(h / 8); i++) js += (i ? "," : "") + std::to_string((unsigned)lv[i]);
        js += "]}";
        FILE *f = fopen(levels_out_file.c_str(), "wb");
        if (!f) die("cannot create " + levels_out_file);
        fwrite(js.data(), 1, js.size(), f);
        fclose(f);
        log_info("Wrote tile levels to " + levels_out_file);
    }
    if (!set_levels_out_file.empty()) { // the ladder and every frame's levels, frames in command-line order
        std::string js = "{\"n\":" + std::to_string(ordered_n) + ",\"amplitudes\":[";
        for (size_t j = 0; j < level_amps.size(); j++) js += (j ? "," : "") + std::to_string(level_amps[j]);
        js += std::string("],\"tied\":") + (set_tied ? "true" : "false") + ",\"frames\":[";
        for (size_t m = 0; m < frames.size(); m++) {
            std::vector<uint8_t> lv(1024);
            if (snesimage_get_tile_levels(frames[m], lv.data()) != 0) die(snesimage_last_error());
            js += m ? ",[" : "[";
            for (size_t i = 0; i < 32 * (size_t)(h / 8); i++) js += (i ? "," : "") + std::to_string((unsigned)lv[i]);
            js += "]";
        }
        js += "]}";
        FILE *f = fopen(set_levels_out_file.c_str(), "wb");
        if (!f) die("cannot create " + set_levels_out_file);
        fwrite(js.data(), 1, js.size(), f);
        fclose(f);
        log_info("Wrote the set's tile levels to " + set_levels_out_file);
    }
    if (!tilemap_file.empty()) {
        const int64_t need = snesimage_as_tilemap_json(ctx, nullptr, 0);
        if (need < 0) die(snesimage_last_error());
        std::vector<char> json((size_t)need);
        snesimage_as_tilemap_json(ctx, json.data(), need);
        FILE *f = fopen(tilemap_file.c_str(), "wb");
        if (!f) die("cannot create " + tilemap_file);
        fwrite(json.data(), 1, (size_t)need - 1, f);
        fclose(f);
        log_info("Wrote tilemap to " + tilemap_file);
    }
    if (!set_tilemap_file.empty()) {
        const int64_t need = snesimage_shared_as_tilemap_json(set, nullptr, 0);
        if (need < 0) die(snesimage_last_error());
        std::vector<char> json((size_t)need);
        snesimage_shared_as_tilemap_json(set, json.data(), need);
        FILE *f = fopen(set_tilemap_file.c_str(), "wb");
        if (!f) die("cannot create " + set_tilemap_file);
        fwrite(json.data(), 1, (size_t)need - 1, f);
        fclose(f);
        log_info("Wrote the set's tilemap to " + set_tilemap_file);
    }
    // The native export, where the tilemap is written.  The bytes are first rendered as the PPU's background fetch reads them
    // (snesimage_render_native) and compared with as_rgba(): equal RGB wherever the source is opaque, CGRAM word 0 elsewhere.
    // A difference is an internal error, and no export file is written.
    if (export_first >= 0 || set_export_first >= 0) {
        const bool of_set = set_export_first >= 0;
        snesimage_native_layout lay{};
        lay.bpp = (uint8_t)export_opt[0].value; lay.char_base = (uint16_t)export_opt[1].value; lay.palette_base = (uint8_t)export_opt[2].value; lay.priority = (uint8_t)export_opt[3].value;
        snesimage_native_info ni{};
        if ((of_set ? snesimage_shared_export_native(set, &lay, nullptr, nullptr, 0, nullptr, &ni) : snesimage_export_native(ctx, &lay, nullptr, nullptr, 0, nullptr, &ni)) != 0)
            die(std::string("Unable to export native data: ") + snesimage_last_error());
        std::vector<uint8_t> cgram(512), chr(ni.chr_bytes);
        std::vector<uint16_t> words(ni.map_words);
        if ((of_set ? snesimage_shared_export_native(set, &lay, cgram.data(), chr.data(), chr.size(), words.data(), &ni)
                    : snesimage_export_native(ctx, &lay, cgram.data(), chr.data(), chr.size(), words.data(), &ni)) != 0 || ni.chr_bytes != chr.size() || ni.map_words != words.size())
            die(std::string("Unable to export native data: ") + snesimage_last_error());
        lay.bpp = (uint8_t)ni.bpp; // the depth the export chose
        const uint32_t ntile = 32 * (h / 8), c0 = (uint32_t)cgram[0] | ((uint32_t)cgram[1] << 8);
        const uint8_t zero[3] = {(uint8_t)((c0 & 31) * 8 + (c0 & 31) / 4), (uint8_t)(((c0 >> 5) & 31) * 8 + ((c0 >> 5) & 31) / 4), (uint8_t)(((c0 >> 10) & 31) * 8 + ((c0 >> 10) & 31) / 4)};
        std::vector<uint8_t> drawn((size_t)w * h * 4), want((size_t)w * h * 4);
        for (size_t m = 0; m < (of_set ? frames.size() : (size_t)1); m++) {
            if (snesimage_render_native(frames[m], &lay, cgram.data(), chr.data(), chr.size(), words.data() + m * ntile, drawn.data()) != 0 || snesimage_as_rgba(frames[m], want.data()) != 0)
                die(std::string("Unable to check the native export: ") + snesimage_last_error());
            for (size_t px = 0; px < (size_t)w * h; px++) {
                const uint8_t *d = &drawn[4 * px], *e = want[4 * px + 3] ? &want[4 * px] : zero; // (as_rgba leaves alpha 0 exactly where the source does)
                if (d[0] != e[0] || d[1] != e[1] || d[2] != e[2] || d[3] != 255)
                    die("internal error: the native export of frame " + std::to_string(m) + " does not render as the result at pixel (" + std::to_string(px % w) + ", " + std::to_string(px / w) + "); nothing was exported");
            }
        }
        const std::string *files = of_set ? set_export_file : export_file;
        const void *data[3] = {cgram.data(), chr.data(), words.data()};
        const size_t bytes[3] = {cgram.size(), chr.size(), words.size() * sizeof(uint16_t)}; // (the words are little-endian as the host is)
        for (int k = 0; k < 3; k++) {
            if (files[k].empty()) continue;
            FILE *f = fopen(files[k].c_str(), "wb");
            if (!f) die("cannot create " + files[k]);
            fwrite(data[k], 1, bytes[k], f);
            fclose(f);
        }
        log_info(std::string("Wrote native data") + (of_set ? " of the set: " : ": ") + std::to_string(ni.bpp) + "bpp, " + std::to_string(ni.unique) + " characters at " + std::to_string(lay.char_base) + ", " +
                 std::to_string(ni.map_words) + " tilemap words");
    }
    if (!preview_file.empty()) { // left: source, right: as_rgba() of the result (src/lib.rs:940-957)
        std::vector<uint8_t> result((size_t)w * h * 4), both((size_t)2 * w * h * 4), png;
        if (snesimage_as_rgba(ctx, result.data()) != 0) die(snesimage_last_error());
        for (uint32_t y = 0; y < h; y++) {
            memcpy(&both[(size_t)y * 2 * w * 4], &rgba[(size_t)y * w * 4], (size_t)w * 4);
            memcpy(&both[((size_t)y * 2 + 1) * w * 4], &result[(size_t)y * w * 4], (size_t)w * 4);
        }
        if (!snes_png::encode_rgba(2 * w, h, both.data(), png)) die("cannot encode " + preview_file);
        FILE *pf = fopen(preview_file.c_str(), "wb");
        if (!pf) die("cannot create " + preview_file);
        fwrite(png.data(), 1, png.size(), pf);
        fclose(pf);
        log_info("Wrote preview to " + preview_file);
    }
    if (group) snesimage_group_destroy(group);
    if (set) snesimage_shared_destroy(set);
    for (snesimage_ctx *m : members) snesimage_destroy(m);
    for (size_t i = 1; i < frames.size(); i++) snesimage_destroy(frames[i]);
    return 0;
}
