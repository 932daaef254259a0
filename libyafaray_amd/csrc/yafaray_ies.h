// IES (IESNA LM-63) photometric files: the parser behind createLight's "ieslight".  Host code with no HIP and no dependence on the
// interface: it compiles alone (tests/ies_parse_cases.cpp builds it with the sanitizers).
//
// What it keeps is what IesData::parseIesFile (include/utility/util_ies.h:135-376) leaves behind, quirks included; what it adds is a
// refusal, with the cause and the file's name, wherever the reference would go on with an unread field or index past an array.
#pragma once
#include <string>
#include <vector>

namespace yafies {

enum { kTypeC = 1, kTypeB = 2, kTypeA = 3 };
constexpr int kMaxAngles = 4096;             // per map
constexpr long long kMaxTable = 1ll << 22;   // floats of one table (n_hor * n_vert, after a single horizontal angle was doubled)

struct Data
{
	int type = 0;                  // the photometric type as read (1 C, 2 B, 3 A; the lookup treats every other value like A)
	int n_hor = 0, n_vert = 0;     // after the adjustment of a type-C file with one horizontal angle (a second one at 180)
	std::vector<float> hor, vert;  // the angle maps in degrees, strictly increasing; vert starts at 0 or below (a positive start is subtracted)
	std::vector<float> table;      // candela values as read, row-major by horizontal angle: table[h * n_vert + v]
	float max_rad = 0.f;           // 1 / the largest value: the lookup multiplies by it (util_ies.h:130)
	float max_v_angle = 0.f;       // the largest vertical angle (after the subtraction), in radians
};

// false: `err` says what is wrong with the file, and names it; `out` is then unspecified.
bool parse_text(const std::string &text, const std::string &name, Data &out, std::string &err);
bool parse_file(const std::string &path, Data &out, std::string &err);

} // namespace yafies
