// The Interface-shaped C ABI (include/yafaray_c_api.h) over the MI355X path-tracing core.
//
// Host-side mirror of the reference's control path for ONE render: ParamMap building
// (src/interface/interface.cc:221-310), the type-string factories of RenderEnvironment
// (src/common/environment.cc:367-454 -> Material::factory etc.), the Scene geometry state machine
// (src/common/scene.cc:110-131,283-338), RenderEnvironment::setupScene (environment.cc:679-813)
// and Scene::update (scene.cc:784-894).  Everything per-sample happens on the device (yafgpu.h).
#include "../../include/yafaray_c_api.h"
#include "../../include/yafgpu.h"
#include "yafaray_image.h"
// The IES parser is a source file of its own, with no HIP and nothing of the interface in it, so that tests/ies_parse_cases.cpp builds it
// alone; the library takes it in here and not as an object of its own, so that every build of the interface's host side has it
#include "yafaray_ies.cpp"

#include <hip/hip_runtime.h>

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <limits>
#include <list>
#include <map>
#include <memory>
#include <new>
#include <string>
#include <vector>

namespace {

constexpr double kPi = 3.14159265358979323846;

// ---- ParamMap (include/common/param.h:37-107): strictly typed values, as Parameter::getVal (param.cc:49-53)
struct Param
{
	enum Type { None, Int, Bool, Float, String, Point, Color, Matrix } type = None;
	int i = 0; bool b = false; double f = 0; std::string s; float v[4] = {0, 0, 0, 0};
	float m[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};     // Matrix4, row major
};
struct ParamMap
{
	std::map<std::string, Param> dicc;
	bool get(const std::string &n, int &o) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Int) return false; o = it->second.i; return true; }
	bool get(const std::string &n, bool &o) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Bool) return false; o = it->second.b; return true; }
	bool get(const std::string &n, float &o) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Float) return false; o = (float)it->second.f; return true; }
	bool get(const std::string &n, double &o) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Float) return false; o = it->second.f; return true; }
	bool get(const std::string &n, std::string &o) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::String) return false; o = it->second.s; return true; }
	bool getPoint(const std::string &n, float o[3]) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Point) return false; o[0] = it->second.v[0]; o[1] = it->second.v[1]; o[2] = it->second.v[2]; return true; }
	bool getColor(const std::string &n, float o[3]) const { auto it = dicc.find(n); if(it == dicc.end() || it->second.type != Param::Color) return false; o[0] = it->second.v[0]; o[1] = it->second.v[1]; o[2] = it->second.v[2]; return true; }
};

struct Mesh
{
	std::vector<float> points;        // xyz
	std::vector<float> normals;       // xyz per vertex (addNormal) or empty
	std::vector<int> tri;             // a,b,c
	std::vector<int> tri_mat;
	bool normals_exported = false, smooth = false, visible = true, base = false;
	std::vector<float> smooth_normals; // per triangle corner, filled by smoothMesh
	bool smooth_by_vertex = false;     // smoothMesh's loop for angle >= 180 gave every corner the normal whose index is its vertex index (scene.cc:420-448)
	// texture coordinates as the exporter gives them (TriangleObject::points_ interleaves orco, uv_values_ / uv_offsets_;
	// object_geom/object_geom_mesh.cc): kept for the shader nodes; untextured shading never reads them
	bool has_orco = false, has_uv = false;
	std::vector<float> orco;          // xyz per vertex
	std::vector<float> uv;            // u, v per addUv
	std::vector<int> tri_uv;          // uv_a, uv_b, uv_c per triangle (when has_uv)
};

// TriangleObjectInstance (object_geom.cc:104-121): the base, obj_to_world and the four flags it copied from the base when it was made
struct Instance
{
	unsigned int base = 0;
	float m[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};     // row major
	bool has_orco = false, has_uv = false, smooth = false, normals_exported = false;
};

// A curve (strand) mesh as Scene::startCurveMesh .. endCurveMesh take it (scene.cc:133-281): the poly-line, one material and the three
// strand parameters.  No triangles are stored: the device extrudes the points at scene set-up (yafgpu_instancing's curve segments).
struct Curve
{
	std::vector<float> points;        // xyz
	std::vector<float> scales;        // h, s per point (curve_scales), filled by endCurveMesh
	int mat = -1;
	float strand_start = 0.f, strand_end = 0.f, strand_shape = 0.f;
};

struct IntegratorCfg
{
	std::string type;
	int path_samples = 32, bounces = 3, rr_min_bounces = 0, raydepth = 5;
	bool no_recursive = false, bg_transp = false, bg_transp_refract = false, transp_shad = false;
	bool trace_caustics = false;     // PathIntegrator: caustic_type_ is Path unless the parameter says "none" (integrator_path_tracer.cc:36, :85, :382-387)
	int shadow_depth = 5;            // integrator_path_tracer.cc:352, integrator_direct_light.cc:201
	// ambient occlusion (integrator_direct_light.cc:200-207,220-223; integrator_path_tracer.cc:355-358,375-378 reads the same four, for
	// render passes this path does not have): only directlighting's integrate() uses it (:145)
	bool do_ao = false;
	int ao_samples = 32;
	float ao_distance = 1.f;         // read as double, kept as float (ao_dist_)
	float ao_color[3] = {1.f, 1.f, 1.f};
};

struct CameraCfg { yafgpu_camera cam; };
struct BackgroundCfg { float color[3]; yafgpu_background rec; yafgpu_sky sky; };      // color: the constant colour (yafgpu_render_params::background); rec, sky: what the device scene gets (sky: a gradient's or a sunsky's constants, else zero)

} // namespace

struct yafaray_material { yafgpu_material m; int index; std::vector<yafgpu_node> nodes; int mask_sub[2] = {-1, -1}; };   // nodes: evaluation order, `texture` = index into texture_order; mask_sub: a mask_mat's material1 / material2 (their `index`)
static_assert(sizeof(yafgpu_material) == 384, "yafaray_getMaterialTable hands out 96-word records");
struct yafaray_texture { yafgpu_texture t; int index; std::vector<float> texels; };            // texels: height * width * 4, as ImageHandler::getPixel returns them
struct yafaray_light { yafgpu_light l; unsigned int object = 0; yafies::Data ies; };      // object: a mesh light's or a portal's mesh (obj_id_ / object_id_), resolved at prepareRender; ies: an ieslight's parsed file
// An image handler made for output (TgaHandler / HdrHandler / PngHandler after initForOutput): the image an output fills and the encoder
// that saves it.  `packed` is what the encoder takes, four bytes a pixel (RGBA8 for tga and png, RGBE for hdr): the device's output stage
// writes it whole; a caller that delivers pixel by pixel fills `rgba` instead, which flush packs on the host (`driven`)
struct yafaray_image_handler
{
	enum Type { Tga, Hdr, Png } type = Tga;
	int width = 0, height = 0; bool alpha = false, for_output = true;
	std::vector<uint8_t> packed;       // height * width * 4
	std::vector<float> rgba;           // height * width * 4, made at the first putPixel
	bool driven = false;
};
// ImageOutput (common/output_image.cc): a handler, the file name and the border; `table` is what yafaray_imageOutputCallbacks hands out
struct yafaray_image_output
{
	std::shared_ptr<yafaray_image_handler> ih;
	std::string path, err;
	int bx = 0, by = 0;
	yafaray_output_t table{};
};
// The device's output stage (yafgpu_output.hip, and the scene's half of it in the device unit).  Weak: a build of the host side without the
// device unit (the sanitizer build's stub) still links and loads, and an image output then fails with "no device unit"
extern "C" int yafgpu_film_to_image(const float *d_film, const yafgpu_image_desc *desc, void *d_image, void *stream) __attribute__((weak));
extern "C" int yafgpu_scene_film_to_image(yafgpu_scene_t *scene, const yafgpu_image_desc *desc, void *h_image) __attribute__((weak));
struct yafaray_camera { CameraCfg c; };
struct yafaray_background { BackgroundCfg b; };
struct yafaray_integrator { IntegratorCfg c; };

struct yafaray_interface
{
	std::string err;
	ParamMap params;
	std::list<ParamMap> eparams;
	ParamMap *cparams = &params;
	// registries, name -> object (environment.h:85-95)
	std::map<std::string, std::unique_ptr<yafaray_material>> materials;
	std::vector<yafaray_material *> material_order;
	std::map<std::string, std::unique_ptr<yafaray_texture>> textures;
	std::vector<yafaray_texture *> texture_order;
	std::string base_dir;                // where relative texture file names are looked up after the working directory (the XML file's directory)
	std::map<std::string, std::unique_ptr<yafaray_light>> lights;
	std::vector<yafaray_light *> light_order;
	std::map<std::string, std::unique_ptr<yafaray_camera>> cameras;
	std::map<std::string, std::unique_ptr<yafaray_background>> backgrounds;
	std::map<std::string, std::unique_ptr<yafaray_integrator>> integrators;
	std::map<std::string, std::shared_ptr<yafaray_image_handler>> image_handlers;      // shared with the image outputs made from them
	std::vector<std::shared_ptr<yafaray_image_handler>> loose_image_handlers;          // createImageHandler with add_to_table = false
	// scene state (scene.cc:110-131): 0 ready, 1 geometry, 2 object; 3 is the reference's object state too, with a curve as the open object
	int state = -1;
	std::map<unsigned int, Mesh> meshes;
	std::map<unsigned int, Instance> instances;      // object ids are shared with meshes: the id decides the place in the flattening order
	std::map<unsigned int, Curve> curves;            // object ids shared with meshes and instances
	Mesh *cur = nullptr, *last = nullptr;   // last: Scene's cur_obj_ outlives endTriMesh (smoothMesh(0, angle))
	Curve *cur_curve = nullptr;             // the open curve (state 3)
	unsigned int cur_curve_id = 0;
	bool last_is_curve = false;             // Scene's cur_obj_ is a curve: smoothMesh(0, angle) would mean it
	unsigned int next_id = 1;
	bool geometry_changed = true;
	// render
	yafgpu_scene_t *gpu = nullptr;
	yafgpu_render_params rp{};
	yafgpu_aa_schedule aa{};
	std::vector<int32_t> resampled;      // pixels sampled by each pass of the last render
	bool prepared = false;
	bool scene_dirty = true;            // something the device scene is made of changed since it was built (Scene::update's state_.changes_, scene.cc:784-790)
	yafgpu_camera scene_cam{}; int scene_threads = 0;
	std::string scene_background;       // the background the device scene was built with (background_name; empty: none)
	int shard_index = 0, shard_count = 1;
	std::vector<float> film;
	yafaray_render_stats_t stats{};
	// libc state behind the tile seeds of the Russian-roulette streams (integrator_tiled.cc:319): the reference's last
	// Material / ObjectGeometric constructor calls srand(its running index) and then draws a random colour
	// (material.cc:53-66, object_geom.cc:39-51); whichever object was made last leaves the state rand() continues from
	uint32_t last_srand = 0u; bool have_srand = false;
	int pass_pipelining = -1;            // yafaray_setPassPipelining: -1 by size, 0 off, 1 on (yafgpu_scene_set_pass_pipelining)
	int user_srand = -1, user_skip = 0;  // yafaray_setRandState: the embedder's own srand() after the last constructor
	bool serial_replay = true;           // yafaray_setSerialReplay
	std::vector<int32_t> tile_rand0;     // the first pass's value per tile (yafaray_renderPassDevice)
	yafgpu_exchange_fn exchange = nullptr; void *exchange_user = nullptr;     // yafaray_setPlaneExchange
	volatile int32_t abort_flag = 0;     // Scene::abort: set by yafaray_abort (any thread), polled by the device side between chunks and passes
	std::string color_space = "Raw_Manual_Gamma"; float gamma = 1.f;
	std::string color_space2 = "Raw_Manual_Gamma"; float gamma2 = 1.f;
	// Interface::setInputColorSpace (interface.cc:292-301): how paramsSetColor reads its arguments; the ctor's default is
	// RawManualGamma with gamma 1 (interface.cc:73), i.e. values are taken as linear
	int input_color_space = 3; float input_gamma = 1.f;       // 0 sRGB, 1 XYZ (D65), 2 LinearRGB, 3 RawManualGamma
	yafaray_output_t output2{}; bool has_output2 = false;
	bool interactive = false; std::string badge_position = "none";
	// film files (yafaray_setFilmPath): the stand-in for session__.getPathImageOutput(), and what the last render loaded
	std::string film_path;
	int film_n_loaded = 0; uint32_t film_sampling_offset = 0u, film_base_sampling_offset = 0u;
};

namespace {

bool fail(yafaray_interface *yi, const std::string &m) { yi->err = m; return false; }

// fPow__ = fExp2__(fLog2__(a) * b), util_math_optimizations.h:116-142,176-183 (FAST_MATH is on in the reference's build)
float host_fexp2(float x)
{
	x = std::min(x, 129.00000f);
	x = std::max(x, -126.99999f);
	const int ipart = (int)(x - 0.5f);
	const float p = (x - (float)ipart);
	const int bits = (int)((unsigned)(ipart + 127) << 23);
	float expi; std::memcpy(&expi, &bits, 4);
	const float poly = (p * (p * (p * (p * (p * 1.8775767e-3f + 8.9893397e-3f) + 5.5826318e-2f) + 2.4015361e-1f) + 6.9315308e-1f) + 9.9999994e-1f);
	return expi * poly;
}
float host_flog2(float x)
{
	int i; std::memcpy(&i, &x, 4);
	const float e = (float)(((i & 0x7F800000) >> 23) - 127);
	const int mi = (i & 0x7FFFFF) | 0x3F800000;
	float m; std::memcpy(&m, &mi, 4);
	const float a = m * -3.4436006e-2f + 3.1821337e-1f;
	const float b = m * a + -1.2315303f;
	const double c = (double)(m * b) + 2.5988452;
	const double d = (double)m * c + (double)-3.3241990f;
	const double ee = (double)m * d + (double)3.1157899f;
	return ((float)ee * (m - 1.0f) + e);
}
float host_fpow(float a, float b) { return host_fexp2(host_flog2(a) * b); }

// Material::material_index_auto_ / ObjectGeometric::object_index_auto_ (common/material.cc:33, object_geom.cc:29): static,
// process-wide, never reset — like the reference, one process is assumed to build its scenes one after the other
unsigned int g_material_index_auto = 0u, g_object_index_auto = 0u;
void note_srand(yafaray_interface *yi, unsigned int seed) { yi->last_srand = seed; yi->have_srand = true; yi->user_srand = -1; yi->user_skip = 0; }
// values the constructor's colour loop consumed after its srand(): do { r, g, b = rand() % 8 / 8 } while(r + g + b < 0.5)
int colour_loop_draws(uint32_t seed)
{
	int32_t v[3 * 64];
	yafgpu_glibc_rand(seed, 3 * 64, v);
	for(int k = 0; k < 64; ++k)
	{
		const float r = (float)(v[3 * k] % 8) / 8.f, g = (float)(v[3 * k + 1] % 8) / 8.f, b = (float)(v[3 * k + 2] % 8) / 8.f;
		if(!(r + g + b < 0.5f)) return 3 * (k + 1);
	}
	return 3 * 64;
}

inline void cross3(const float a[3], const float b[3], float o[3]) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
inline void normalize3(float v[3]) // Vec3::normalize, vector.h:227-238
{
	float len = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
	if(len != 0.f) { len = 1.0f / std::sqrt(len); v[0] *= len; v[1] *= len; v[2] *= len; }
}

int visibility_from(const std::string &s)
{
	if(s == "no_shadows") return 1;
	if(s == "shadow_only") return 2;
	if(s == "invisible") return 3;
	return 0;
}


// ---- shader nodes -----------------------------------------------------------------------------------
inline void clear_shader_slots(yafgpu_material &m)
{
	m.node_first = 0; m.n_nodes = 0;
	m.sh_diffuse = m.sh_mirror_color = m.sh_mirror = m.sh_transparency = m.sh_translucency = m.sh_sigma_oren = m.sh_diffuse_refl = m.sh_ior = -1;
	m.sh_glossy = m.sh_glossy_reflect = m.sh_exponent = m.sh_filter_color = -1;
	m.bump_first = 0; m.n_bump = 0; m.sh_bump = -1;
}

constexpr int kMaxMaterialNodes = 16;    // yafgpu_texture.h kMaxNodes: the per-lane node stack of the shading kernels

struct LoadedNodes
{
	std::vector<yafgpu_node> nodes;                 // as listed (loadNodes order), references = indices into this list
	std::map<std::string, int> by_name;
};

// the four factories + configInputs (shader_node.cc:28-37; shader_node_basic.cc:345-409, :425-434, :482-531, :683-703;
// shader_node_layer.cc:162-201, :211-245).  -1 = the reference's own failure (it then builds the material without shaders,
// material_shiny_diffuse.cc:709-713), 0 = refused by the GPU path (err set), 1 = loaded
int load_nodes(yafaray_interface *yi, const std::list<ParamMap> &list, LoadedNodes &out)
{
	if(list.size() > 4096) { fail(yi, "shader nodes: more than 4096 nodes in one material's list"); return 0; }      // (sort_nodes walks the graph recursively)
	std::vector<const ParamMap *> maps;
	for(const ParamMap &pm : list)
	{	// NodeMaterial::loadNodes, material_node.cc:150-205
		std::string element, name, type;
		if(pm.get("element", element) && element != "shader_node") continue;
		if(!pm.get("name", name)) return -1;
		if(out.by_name.count(name)) return -1;
		if(!pm.get("type", type)) return -1;
		yafgpu_node n; std::memset(&n, 0, sizeof n);
		n.texture = n.input1 = n.input2 = n.factor = n.input = n.upper = -1;
		if(type == "texture_mapper")
		{
			n.type = YAFGPU_NODE_TEXTURE_MAPPER;
			std::string texname, option;
			if(!pm.get("texture", texname)) return -1;
			auto tex = yi->textures.find(texname);
			if(tex == yi->textures.end()) return -1;
			n.texture = tex->second->index;
			n.texco = 1;         // Coords { Uv, Glob, Orco, Tran, Nor, Refl, Win, Stick, Stress, Tan }, shader_node_basic.h
			if(pm.get("texco", option))
			{
				static const char *names[] = {"uv", "global", "orco", "transformed", "normal", "reflect", "window", "stick", "stress", "tangent"};
				for(int k = 0; k < 10; ++k) if(option == names[k]) n.texco = k;
			}
			n.mapping = 0;       // Projection { Plain, Cube, Tube, Sphere }; image textures are discrete()
			if(pm.get("mapping", option))
			{
				static const char *names[] = {"plain", "cube", "tube", "sphere"};
				for(int k = 0; k < 4; ++k) if(option == names[k]) n.mapping = k;
			}
			float scale[3] = {1, 1, 1}, offset[3] = {0, 0, 0}; bool scalar = true; int map[3] = {1, 2, 3};
			for(int k = 0; k < 16; ++k) n.mtx[k] = (k % 5 == 0) ? 1.f : 0.f;
			{ auto it = pm.dicc.find("transform"); if(it != pm.dicc.end() && it->second.type == Param::Matrix) std::memcpy(n.mtx, it->second.m, sizeof n.mtx); }
			pm.getPoint("scale", scale); pm.getPoint("offset", offset); pm.get("do_scalar", scalar);
			pm.get("proj_x", map[0]); pm.get("proj_y", map[1]); pm.get("proj_z", map[2]);
			for(int k = 0; k < 3; ++k) map[k] = std::min(3, std::max(0, map[k]));
			n.map_x = map[0]; n.map_y = map[1]; n.map_z = map[2];
			for(int k = 0; k < 3; ++k) { n.scale[k] = scale[k]; n.offset[k] = 2 * offset[k]; }
			n.do_scalar = scalar ? 1 : 0;
			{	// setup(), shader_node_basic.cc:34-59 (image textures are discrete; normal maps are refused at createTexture)
				float bump_str = 1.f; pm.get("bump_strength", bump_str);
				const yafgpu_texture &t = tex->second->t;
				n.d_u = 1.f / (float)t.width; n.d_v = 1.f / (float)t.height;
				bump_str /= std::sqrt(scale[0] * scale[0] + scale[1] * scale[1] + scale[2] * scale[2]);
				if(!t.normalmap) bump_str /= 100.0f;
				n.bump_str = bump_str;
			}
		}
		else if(type == "value")
		{
			n.type = YAFGPU_NODE_VALUE;
			float col[3] = {1, 1, 1}, alpha = 1.f, val = 1.f;
			pm.getColor("color", col); pm.get("alpha", alpha); pm.get("scalar", val);
			n.color[0] = col[0]; n.color[1] = col[1]; n.color[2] = col[2]; n.color[3] = alpha; n.value = val;
		}
		else if(type == "mix")
		{
			n.type = YAFGPU_NODE_MIX;
			float val = 0.5f; int mode = 0;
			pm.get("cfactor", val); pm.get("mode", mode);
			// MixNode::factory's switch has no case for MnDiv (5) and none above MnOverlay (9): those build a plain MixNode
			n.mode = (mode >= 0 && mode <= 9 && mode != 5) ? mode : 0;
			n.cfactor = (n.mode == 0) ? val : 0.f;       // MixNode(val) / the derived nodes' MixNode(): cfactor_ 0
			n.col1[3] = n.col2[3] = 1.f;
		}
		else if(type == "layer")
		{
			n.type = YAFGPU_NODE_LAYER;
			float def_col[3] = {1, 1, 1};
			bool do_color = true, do_scalar = false, color_input = true, use_alpha = false, stencil = false, no_rgb = false, negative = false;
			double def_val = 1.0, colfac = 1.0, valfac = 1.0; int mode = 0;
			pm.get("mode", mode); pm.getColor("def_col", def_col); pm.get("colfac", colfac); pm.get("def_val", def_val); pm.get("valfac", valfac);
			pm.get("do_color", do_color); pm.get("do_scalar", do_scalar); pm.get("color_input", color_input); pm.get("use_alpha", use_alpha);
			pm.get("noRGB", no_rgb); pm.get("stencil", stencil); pm.get("negative", negative);
			n.texflag = (no_rgb ? 1u : 0u) | (stencil ? 2u : 0u) | (negative ? 4u : 0u) | (use_alpha ? 8u : 0u);
			n.mode = mode; n.colfac = (float)colfac; n.valfac = (float)valfac; n.def_val = (float)def_val;
			n.def_col[0] = def_col[0]; n.def_col[1] = def_col[1]; n.def_col[2] = def_col[2]; n.def_col[3] = 1.f;
			n.do_color = do_color; n.do_scalar_l = do_scalar; n.color_input = color_input; n.use_alpha = use_alpha;
		}
		else return -1;      // ShaderNode::factory knows no other type: "No shader node was constructed by plugin"
		out.by_name[name] = (int)out.nodes.size();
		out.nodes.push_back(n);
		maps.push_back(&pm);
	}
	for(size_t k = 0; k < out.nodes.size(); ++k)
	{	// configInputs, material_node.cc:207-220
		yafgpu_node &n = out.nodes[k]; const ParamMap &pm = *maps[k];
		auto find = [&](const std::string &nm) { auto it = out.by_name.find(nm); return it == out.by_name.end() ? -1 : it->second; };
		auto rgba = [&](const char *key, float o[4]) { auto it = pm.dicc.find(key); if(it == pm.dicc.end() || it->second.type != Param::Color) return false; for(int c = 0; c < 4; ++c) o[c] = it->second.v[c]; return true; };
		std::string name;
		if(n.type == YAFGPU_NODE_MIX)
		{
			if(pm.get("input1", name)) { if((n.input1 = find(name)) < 0) return -1; }
			else if(!rgba("color1", n.col1)) return -1;
			if(pm.get("input2", name)) { if((n.input2 = find(name)) < 0) return -1; }
			else if(!rgba("color2", n.col2)) return -1;
			if(pm.get("factor", name)) { if((n.factor = find(name)) < 0) return -1; }
			else if(!pm.get("value", n.cfactor)) return -1;
		}
		else if(n.type == YAFGPU_NODE_LAYER)
		{
			if(!pm.get("input", name)) return -1;
			if((n.input = find(name)) < 0) return -1;
			if(pm.get("upper_layer", name)) { if((n.upper = find(name)) < 0) return -1; }
			else
			{
				n.upper_col[3] = 1.f;
				if(!rgba("upper_color", n.upper_col)) { n.upper_col[0] = n.upper_col[1] = n.upper_col[2] = 0.f; n.upper_col[3] = 1.f; }
				if(!pm.get("upper_value", n.upper_val)) n.upper_val = 0.f;
			}
		}
	}
	return 1;
}

// NodeMaterial::solveNodesOrder + getNodeList (material_node.cc:88-121): the nodes the material's shader slots reach, every node
// after the ones it reads.  slots: in = index into ld.nodes or -1, out = index into `sorted`.  false: a cycle, or more nodes
// than the shading kernels' stack holds (err set).
bool sort_nodes(yafaray_interface *yi, const LoadedNodes &ld, int *slots, int n_slots, std::vector<yafgpu_node> &sorted)
{
	const int n = (int)ld.nodes.size();
	std::vector<int> new_index((size_t)n, -1), mark((size_t)n, 0);
	std::vector<int> order;
	bool cycle = false;
	std::function<void(int)> visit = [&](int k)
	{
		if(k < 0 || mark[(size_t)k] == 2) return;
		if(mark[(size_t)k] == 1) { cycle = true; return; }
		mark[(size_t)k] = 1;
		const yafgpu_node &nd = ld.nodes[(size_t)k];
		visit(nd.input1); visit(nd.input2); visit(nd.factor); visit(nd.input); visit(nd.upper);
		mark[(size_t)k] = 2;
		new_index[(size_t)k] = (int)order.size(); order.push_back(k);
	};
	for(int s = 0; s < n_slots; ++s) visit(slots[s]);
	if(cycle) return fail(yi, "shader nodes: the node graph has a cycle");
	if((int)order.size() > kMaxMaterialNodes) return fail(yi, "shader nodes: more than 16 nodes reachable from one material's shader slots is not supported by the GPU path");
	auto remap = [&](int k) { return k < 0 ? -1 : new_index[(size_t)k]; };
	sorted.clear();
	for(int k : order)
	{
		yafgpu_node nd = ld.nodes[(size_t)k];
		nd.input1 = remap(nd.input1); nd.input2 = remap(nd.input2); nd.factor = remap(nd.factor); nd.input = remap(nd.input); nd.upper = remap(nd.upper);
		sorted.push_back(nd);
	}
	for(int s = 0; s < n_slots; ++s) slots[s] = remap(slots[s]);
	return true;
}

// NodeMaterial's bump_nodes_ (getNodeList(bump_shader_, bump_nodes_), material_shiny_diffuse.cc:746, material_glossy.cc:545, ...): what the
// bump shader reaches, in evaluation order, kept behind the material's colour nodes.  first / count / slot: relative to `nodes`.
struct BumpList { int first = 0, count = 0, slot = -1; };
bool append_bump_nodes(yafaray_interface *yi, const LoadedNodes &ld, int bump_slot, std::vector<yafgpu_node> &nodes, BumpList &out)
{
	out = BumpList();
	if(bump_slot < 0) return true;
	std::vector<yafgpu_node> bump; int slot[1] = {bump_slot};
	if(!sort_nodes(yi, ld, slot, 1, bump)) return false;
	out.first = (int)nodes.size(); out.count = (int)bump.size(); out.slot = slot[0];
	nodes.insert(nodes.end(), bump.begin(), bump.end());
	return true;
}

// ShinyDiffuseMaterial::factory + ctor + config, material_shiny_diffuse.cc:599-690, :26-36, :46-92
bool make_shinydiffuse(yafaray_interface *yi, const ParamMap &p, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	float color[3] = {1, 1, 1}, mirror_color[3] = {1, 1, 1};
	float diffuse = 1.f, transp = 0.f, transl = 0.f, mirror = 0.f, emit = 0.f, ior = 1.33f, wire = 0.f;
	bool fresnel = false, recv = true, flat = false;
	double transmit_filter = 1.0;
	std::string vis = "normal", brdf;
	p.getColor("color", color); p.getColor("mirror_color", mirror_color);
	p.get("transparency", transp); p.get("translucency", transl); p.get("diffuse_reflect", diffuse);
	p.get("specular_reflect", mirror); p.get("emit", emit); p.get("IOR", ior); p.get("fresnel_effect", fresnel);
	p.get("transmit_filter", transmit_filter); p.get("receive_shadows", recv); p.get("flat_material", flat);
	p.get("visibility", vis); p.get("wireframe_amount", wire);
	if(wire != 0.f) return fail(yi, "shinydiffusemat: wireframe shading is not supported by the GPU path");
	// recursiveRaytrace's per-material parameters (integrator_montecarlo.cc:791, :1003-1014).  (`samplingfactor` only feeds a debug
	// render pass, integrator_tiled.cc:597.)
	int add_depth = 0; float tb_factor = 0.f; bool tb_mult = false;
	p.get("additionaldepth", add_depth); p.get("transparentbias_factor", tb_factor); p.get("transparentbias_multiply_raydepth", tb_mult);
	if(add_depth < 0 || add_depth > 7) return fail(yi, "shinydiffusemat: additionaldepth outside [0, 7]: the device path keeps at most 7 recursion frames per sample");
	// shader nodes, material_shiny_diffuse.cc:692-747: slots in the order of yafgpu_material's sh_* fields
	enum { kDiffuse, kMirrorColor, kMirror, kTransparency, kTranslucency, kSigmaOren, kDiffuseRefl, kIor, kBump, kWireframe, kSlots };
	int slots[kSlots]; for(int &v : slots) v = -1;
	int n_color_nodes = 0; BumpList bump;
	nodes.clear();
	if(!yi->eparams.empty())
	{
		LoadedNodes ld;
		const int rc = load_nodes(yi, yi->eparams, ld);
		if(rc == 0) return false;
		if(rc > 0)
		{	// parseNodes, material_node.cc:227-247: a slot naming a node that does not exist stays empty
			static const char *names[kSlots] = {"diffuse_shader", "mirror_color_shader", "mirror_shader", "transparency_shader", "translucency_shader",
			                                    "sigma_oren_shader", "diffuse_refl_shader", "IOR_shader", "bump_shader", "wireframe_shader"};
			std::string node;
			for(int k = 0; k < kSlots; ++k) if(p.get(names[k], node)) { auto it = ld.by_name.find(node); if(it != ld.by_name.end()) slots[k] = it->second; }
			if(slots[kWireframe] >= 0) return fail(yi, "shinydiffusemat: wireframe_shader is not supported by the GPU path");
			const int bump_slot = slots[kBump]; slots[kBump] = -1;
			if(!sort_nodes(yi, ld, slots, kSlots, nodes)) return false;
			n_color_nodes = (int)nodes.size();
			if(!append_bump_nodes(yi, ld, bump_slot, nodes, bump)) return false;
		}
		else std::fprintf(stderr, "WARNING: ShinyDiffuse: Loading shader nodes failed! (the material is built without them, as the reference does)\n");
	}
	std::memset(&m, 0, sizeof m);
	clear_shader_slots(m);
	m.n_nodes = (int32_t)n_color_nodes; m.bump_first = bump.first; m.n_bump = bump.count; m.sh_bump = bump.slot;
	m.sh_diffuse = slots[kDiffuse]; m.sh_mirror_color = slots[kMirrorColor]; m.sh_mirror = slots[kMirror]; m.sh_transparency = slots[kTransparency];
	m.sh_translucency = slots[kTranslucency]; m.sh_sigma_oren = slots[kSigmaOren]; m.sh_diffuse_refl = slots[kDiffuseRefl]; m.sh_ior = slots[kIor];
	m.ior_base = ior; m.emit_strength = emit;
	m.additional_depth = add_depth; m.transp_bias_factor = tb_factor; m.transp_bias_mult = tb_mult ? 1 : 0;
	m.type = YAFGPU_MAT_SHINYDIFFUSE; m.visibility = visibility_from(vis); m.receive_shadows = recv; m.flat = flat;
	for(int k = 0; k < 3; ++k) { m.diffuse_color[k] = color[k]; m.mirror_color[k] = mirror_color[k]; m.emit_color[k] = emit * color[k]; }
	m.diffuse_strength = diffuse; m.transparency_strength = transp; m.translucency_strength = transl; m.mirror_strength = mirror;
	m.transmit_filter = (float)transmit_filter;
	m.bsdf_flags = 0u;
	if(emit > 0.f) m.bsdf_flags |= 0x80u;
	m.ior_squared = 1.f;
	if(fresnel) { m.ior_squared = ior * ior; m.has_fresnel = 1; }
	if(p.get("diffuse_brdf", brdf) && brdf == "oren_nayar")
	{	// initOrenNayar :190-196
		double sigma = 0.1; p.get("sigma", sigma);
		const double s2 = sigma * sigma;
		m.oren_a = (float)(1.0 - 0.5 * (s2 / (s2 + 0.33)));
		m.oren_b = (float)(0.45 * s2 / (s2 + 0.09));
		m.use_oren = 1;
	}
	float acc = 1.f;
	m.n_bsdf = 0;
	if(m.mirror_strength > 0.00001f || m.sh_mirror >= 0)
	{
		m.is_mirror = 1;
		if(m.sh_mirror >= 0) {}
		else if(!m.has_fresnel) acc = 1.f - m.mirror_strength;
		m.bsdf_flags |= 0x1u | 0x10u;
		m.c_flags[m.n_bsdf] = 0x1u | 0x10u; m.c_index[m.n_bsdf] = 0; ++m.n_bsdf;
	}
	if(m.transparency_strength * acc > 0.00001f || m.sh_transparency >= 0)
	{
		m.is_transparent = 1;
		if(m.sh_transparency < 0) acc *= 1.f - m.transparency_strength;
		m.bsdf_flags |= 0x20u | 0x40u;
		m.c_flags[m.n_bsdf] = 0x20u | 0x40u; m.c_index[m.n_bsdf] = 1; ++m.n_bsdf;
	}
	if(m.translucency_strength * acc > 0.00001f || m.sh_translucency >= 0)
	{
		m.is_translucent = 1;
		if(m.sh_translucency < 0) acc *= 1.f - m.transparency_strength; // sic, material_shiny_diffuse.cc:72
		m.bsdf_flags |= 0x4u | 0x20u;
		m.c_flags[m.n_bsdf] = 0x4u | 0x20u; m.c_index[m.n_bsdf] = 2; ++m.n_bsdf;
	}
	if(m.diffuse_strength * acc > 0.00001f)
	{
		m.is_diffuse = 1;
		m.bsdf_flags |= 0x4u | 0x10u;
		m.c_flags[m.n_bsdf] = 0x4u | 0x10u; m.c_index[m.n_bsdf] = 3; ++m.n_bsdf;
	}
	return true;
}

// shader slots of glossy / coated_glossy (material_glossy.cc:490-530, material_coated_glossy.cc:556-602): loads the node list, maps the
// named slots and keeps what they reach in evaluation order.  false: refused (err set).
bool glossy_nodes(yafaray_interface *yi, const ParamMap &p, const char *what, bool coated, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	enum { kDiffuse, kGlossy, kGlossyReflect, kSigmaOren, kExponent, kDiffuseRefl, kIor, kMirror, kMirrorColor, kBump, kWireframe, kSlots };
	static const char *names[kSlots] = {"diffuse_shader", "glossy_shader", "glossy_reflect_shader", "sigma_oren_shader", "exponent_shader", "diffuse_refl_shader",
	                                    "IOR_shader", "mirror_shader", "mirror_color_shader", "bump_shader", "wireframe_shader"};
	int slots[kSlots]; for(int &v : slots) v = -1;
	nodes.clear();
	clear_shader_slots(m);
	if(yi->eparams.empty()) return true;
	LoadedNodes ld;
	const int rc = load_nodes(yi, yi->eparams, ld);
	if(rc == 0) return false;
	if(rc < 0) { std::fprintf(stderr, "WARNING: %s: Loading shader nodes failed! (the material is built without them, as the reference does)\n", what); return true; }
	std::string node;
	for(int k = 0; k < kSlots; ++k)
	{
		if(!coated && (k == kIor || k == kMirror || k == kMirrorColor)) continue;       // glossy has no such slots
		if(p.get(names[k], node)) { auto it = ld.by_name.find(node); if(it != ld.by_name.end()) slots[k] = it->second; }
	}
	if(slots[kWireframe] >= 0) return fail(yi, std::string(what) + ": wireframe_shader is not supported by the GPU path");
	const int bump_slot = slots[kBump]; slots[kBump] = -1;
	if(!sort_nodes(yi, ld, slots, kSlots, nodes)) return false;
	m.n_nodes = (int32_t)nodes.size();
	BumpList bump;
	if(!append_bump_nodes(yi, ld, bump_slot, nodes, bump)) return false;
	m.bump_first = bump.first; m.n_bump = bump.count; m.sh_bump = bump.slot;
	m.sh_diffuse = slots[kDiffuse]; m.sh_glossy = slots[kGlossy]; m.sh_glossy_reflect = slots[kGlossyReflect]; m.sh_sigma_oren = slots[kSigmaOren];
	m.sh_exponent = slots[kExponent]; m.sh_diffuse_refl = slots[kDiffuseRefl]; m.sh_ior = slots[kIor]; m.sh_mirror = slots[kMirror]; m.sh_mirror_color = slots[kMirrorColor];
	return true;
}

// GlossyMaterial::factory + ctor, material_glossy.cc:407-472, :32-50
bool make_glossy(yafaray_interface *yi, const ParamMap &p, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	float col[3] = {1, 1, 1}, dcol[3] = {1, 1, 1};
	float refl = 1.f, diff = 0.f, exponent = 50.f, wire = 0.f;
	bool as_diff = true, aniso = false, recv = true;
	std::string vis = "normal", brdf;
	p.getColor("color", col); p.getColor("diffuse_color", dcol); p.get("diffuse_reflect", diff); p.get("glossy_reflect", refl);
	p.get("as_diffuse", as_diff); p.get("exponent", exponent); p.get("anisotropic", aniso);
	p.get("receive_shadows", recv); p.get("visibility", vis); p.get("wireframe_amount", wire);
	if(wire != 0.f) return fail(yi, "glossy: wireframe shading is not supported by the GPU path");
	int add_depth = 0; p.get("additionaldepth", add_depth);
	if(add_depth < 0 || add_depth > 7) return fail(yi, "glossy: additionaldepth outside [0, 7]: the device path keeps at most 7 recursion frames per sample");
	std::memset(&m, 0, sizeof m);
	if(!glossy_nodes(yi, p, "glossy", false, m, nodes)) return false;
	m.type = YAFGPU_MAT_GLOSSY; m.visibility = visibility_from(vis); m.receive_shadows = recv;
	m.additional_depth = add_depth;
	for(int k = 0; k < 3; ++k) { m.gloss_color[k] = col[k]; m.diff_color[k] = dcol[k]; }
	m.exponent = exponent; m.reflectivity = refl; m.diffuse = diff; m.as_diffuse = as_diff;
	if(aniso)
	{	// material_glossy.cc:464-472
		float e_u = 50.f, e_v = 50.f;
		p.get("exp_u", e_u); p.get("exp_v", e_v);
		m.anisotropic = 1; m.exp_u = e_u; m.exp_v = e_v;
	}
	m.bsdf_flags = 0u;
	if(diff > 0) { m.bsdf_flags = 0x4u | 0x10u; m.with_diffuse = 1; }
	m.bsdf_flags |= as_diff ? (0x4u | 0x10u) : (0x2u | 0x10u);
	if(p.get("diffuse_brdf", brdf) && brdf == "Oren-Nayar")
	{	// :66-72
		double sigma = 0.1; p.get("sigma", sigma);
		const double s2 = sigma * sigma;
		m.oren_a = (float)(1.0 - 0.5 * (s2 / (s2 + 0.33)));
		m.oren_b = (float)(0.45 * s2 / (s2 + 0.09));
		m.use_oren = 1;
	}
	return true;
}

// LightMaterial::factory, material_simple.cc:63-73
bool make_lightmat(const ParamMap &p, yafgpu_material &m)
{
	float col[3] = {1, 1, 1}; double power = 1.0; bool ds = false;
	p.getColor("color", col); p.get("power", power); p.get("double_sided", ds);
	std::memset(&m, 0, sizeof m);
	m.type = YAFGPU_MAT_LIGHT; m.receive_shadows = 1;
	for(int k = 0; k < 3; ++k) m.light_col[k] = (float)power * col[k];
	m.double_sided = ds;
	m.bsdf_flags = 0x80u;
	return true;
}

// CoatedGlossyMaterial::factory + ctor, material_coated_glossy.cc:464-560, :41-66 (Blinn lobe, as_diffuse only)
bool make_coated_glossy(yafaray_interface *yi, const ParamMap &p, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	float col[3] = {1, 1, 1}, dcol[3] = {1, 1, 1}, mcol[3] = {1, 1, 1};
	float refl = 1.f, diff = 0.f, exponent = 50.f, mirror = 1.f, wire = 0.f; double ior = 1.4, sigma = 0.1;
	bool as_diff = true, aniso = false, recv = true; std::string vis = "normal", brdf; int add_depth = 0;
	p.getColor("color", col); p.getColor("diffuse_color", dcol); p.get("diffuse_reflect", diff); p.get("glossy_reflect", refl);
	p.get("as_diffuse", as_diff); p.get("exponent", exponent); p.get("anisotropic", aniso); p.get("IOR", ior);
	p.getColor("mirror_color", mcol); p.get("specular_reflect", mirror);
	p.get("receive_shadows", recv); p.get("visibility", vis); p.get("additionaldepth", add_depth); p.get("wireframe_amount", wire);
	if(wire != 0.f) return fail(yi, "coated_glossy: wireframe shading is not supported by the GPU path");
	if(add_depth < 0 || add_depth > 7) return fail(yi, "coated_glossy: additionaldepth outside [0, 7]: the device path keeps at most 7 recursion frames per sample");
	if(ior == 1.0) ior = 1.0000001f;                                // :512
	std::memset(&m, 0, sizeof m);
	if(!glossy_nodes(yi, p, "coated_glossy", true, m, nodes)) return false;
	m.ior_base = (float)ior;
	m.type = YAFGPU_MAT_COATED_GLOSSY; m.visibility = visibility_from(vis); m.receive_shadows = recv;
	m.additional_depth = add_depth;
	for(int k = 0; k < 3; ++k) { m.gloss_color[k] = col[k]; m.diff_color[k] = dcol[k]; m.mirror_color[k] = mcol[k]; }
	m.mirror_strength = mirror; m.glass_ior = (float)ior; m.exponent = exponent; m.reflectivity = refl; m.diffuse = diff; m.as_diffuse = as_diff;
	if(aniso)
	{	// material_coated_glossy.cc:529-537
		float e_u = 50.f, e_v = 50.f;
		p.get("exp_u", e_u); p.get("exp_v", e_v);
		m.anisotropic = 1; m.exp_u = e_u; m.exp_v = e_v;
	}
	m.c_flags[0] = 0x1u | 0x10u;                                    // Specular | Reflect
	m.c_flags[1] = as_diff ? (0x4u | 0x10u) : (0x2u | 0x10u);         // :55: as_diffuse ? Diffuse | Reflect : Glossy | Reflect (recursiveRaytrace's glossy branch then samples it)
	if(diff > 0.f) { m.c_flags[2] = 0x4u | 0x10u; m.with_diffuse = 1; m.n_bsdf = 3; }
	else { m.c_flags[2] = 0u; m.n_bsdf = 2; }
	m.bsdf_flags = m.c_flags[0] | m.c_flags[1] | m.c_flags[2];
	if(p.get("diffuse_brdf", brdf) && brdf == "Oren-Nayar")
	{	// initOrenNayar :81-87
		p.get("sigma", sigma);
		const double s2 = sigma * sigma;
		m.oren_a = (float)(1.0 - 0.5 * (s2 / (s2 + 0.33))); m.oren_b = (float)(0.45 * s2 / (s2 + 0.09)); m.use_oren = 1;
	}
	return true;
}

// GlassMaterial::factory + ctor, material_glass.cc:340-443, :32-49 (no dispersion or shader nodes)
bool make_glass(yafaray_interface *yi, const ParamMap &p, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	double ior = 1.4, filt = 0.0, disp = 0.0; float fcol[3] = {1, 1, 1}, scol[3] = {1, 1, 1}, absorp[3] = {1, 1, 1}, wire = 0.f;
	bool fake = false, recv = true; std::string vis = "normal"; int add_depth = 0;
	p.get("IOR", ior); p.getColor("filter_color", fcol); p.get("transmit_filter", filt); p.getColor("mirror_color", scol);
	p.get("dispersion_power", disp); p.get("fake_shadows", fake); p.get("receive_shadows", recv); p.get("visibility", vis);
	p.get("additionaldepth", add_depth); p.get("wireframe_amount", wire); p.getColor("absorption", absorp);
	if(disp > 0.0) return fail(yi, "glass: dispersion is not supported by the GPU path (recursiveRaytrace's dispersive branch)");
	if(add_depth < 0 || add_depth > 7) return fail(yi, "glass: additionaldepth outside [0, 7]: the device path keeps at most 7 recursion frames per sample");
	if(wire != 0.f) return fail(yi, "glass: wireframe shading is not supported by the GPU path");
	std::memset(&m, 0, sizeof m);
	clear_shader_slots(m);
	nodes.clear();
	if(!yi->eparams.empty())
	{	// material_glass.cc:402-441: mirror_color_shader, filter_color_shader, IOR_shader, bump_shader (wireframe refused)
		enum { kMirrorColor, kFilterColor, kIor, kBump, kWireframe, kSlots };
		static const char *names[kSlots] = {"mirror_color_shader", "filter_color_shader", "IOR_shader", "bump_shader", "wireframe_shader"};
		int slots[kSlots]; for(int &v : slots) v = -1;
		LoadedNodes ld;
		const int rc = load_nodes(yi, yi->eparams, ld);
		if(rc == 0) return false;
		if(rc > 0)
		{
			std::string node;
			for(int k = 0; k < kSlots; ++k) if(p.get(names[k], node)) { auto it = ld.by_name.find(node); if(it != ld.by_name.end()) slots[k] = it->second; }
			if(slots[kWireframe] >= 0) return fail(yi, "glass: wireframe_shader is not supported by the GPU path");
			const int bump_slot = slots[kBump]; slots[kBump] = -1;
			if(!sort_nodes(yi, ld, slots, kSlots, nodes)) return false;
			m.n_nodes = (int32_t)nodes.size();
			BumpList bump;
			if(!append_bump_nodes(yi, ld, bump_slot, nodes, bump)) return false;
			m.bump_first = bump.first; m.n_bump = bump.count; m.sh_bump = bump.slot;
			m.sh_mirror_color = slots[kMirrorColor]; m.sh_filter_color = slots[kFilterColor]; m.sh_ior = slots[kIor];
		}
		else std::fprintf(stderr, "WARNING: Glass: Loading shader nodes failed! (the material is built without them, as the reference does)\n");
	}
	m.ior_base = (float)ior; m.transp_ior = (float)ior;
	m.type = YAFGPU_MAT_GLASS; m.receive_shadows = recv; m.visibility = visibility_from(vis);
	m.additional_depth = add_depth;
	m.glass_ior = (float)ior;
	const float ff = (float)filt, fc = (float)(1.f - filt);       // filt * filt_col + Rgb(1.f - filt)
	for(int k = 0; k < 3; ++k) { m.filter_color[k] = ff * fcol[k] + fc; m.mirror_color[k] = scol[k]; }
	m.fake_shadow = fake;
	m.bsdf_flags = 0x1u | 0x10u | 0x20u;                         // BsdfAllSpecular
	if(fake) m.bsdf_flags |= 0x40u;
	m.tm_flags = fake ? (0x40u | 0x20u) : (0x1u | 0x20u);
	if(absorp[0] < 1.f || absorp[1] < 1.f || absorp[2] < 1.f)
	{	// material_glass.cc:371-398: vol_i_ = BeerVolumeHandler(absorption, absorption_dist); volumehandler_beer.cc:28-35
		double dist = 1.0;
		p.get("absorption_dist", dist);
		const float maxlog = (float)std::log(1e38);
		for(int k = 0; k < 3; ++k)
		{
			m.beer_sigma[k] = (absorp[k] > 1e-38) ? (float)-std::log((double)absorp[k]) : maxlog;
			if(dist != 0.f) m.beer_sigma[k] = m.beer_sigma[k] * (float)(1.f / dist);
		}
		m.has_vol_i = 1;
		m.bsdf_flags |= 0x100u;                                   // BsdfVolumetric
	}
	return true;
}
// RoughGlassMaterial::factory + ctor, material_rough_glass.cc:320-455, :33-48 (no dispersion, no shader nodes)
bool make_rough_glass(yafaray_interface *yi, const ParamMap &p, yafgpu_material &m, std::vector<yafgpu_node> &nodes)
{
	float ior = 1.4f, filt = 0.f, alpha = 0.5f, disp = 0.f, fcol[3] = {1, 1, 1}, scol[3] = {1, 1, 1}, absorp[3] = {1, 1, 1}, wire = 0.f;
	bool fake = false, recv = true; std::string vis = "normal", node; int add_depth = 0;
	p.get("IOR", ior); p.getColor("filter_color", fcol); p.get("transmit_filter", filt); p.getColor("mirror_color", scol); p.get("alpha", alpha);
	p.get("dispersion_power", disp); p.get("fake_shadows", fake); p.get("receive_shadows", recv); p.get("visibility", vis);
	p.get("additionaldepth", add_depth); p.get("wireframe_amount", wire); p.getColor("absorption", absorp);
	if(disp > 0.f) return fail(yi, "rough_glass: dispersion is not supported by the GPU path (recursiveRaytrace's dispersive branch)");
	if(add_depth < 0 || add_depth > 7) return fail(yi, "rough_glass: additionaldepth outside [0, 7]: the device path keeps at most 7 recursion frames per sample");
	if(wire != 0.f) return fail(yi, "rough_glass: wireframe shading is not supported by the GPU path");
	for(const char *name : {"mirror_color_shader", "bump_shader", "filter_color_shader", "IOR_shader", "wireframe_shader", "roughness_shader"})
		if(p.get(name, node)) return fail(yi, std::string("rough_glass: ") + name + " is not supported by the GPU path (shader nodes on rough glass)");
	std::memset(&m, 0, sizeof m);
	clear_shader_slots(m);
	nodes.clear();
	alpha = std::max(1e-4f, std::min(alpha * 0.5f, 1.f));          // :375
	m.type = YAFGPU_MAT_ROUGH_GLASS; m.receive_shadows = recv; m.visibility = visibility_from(vis);
	m.additional_depth = add_depth;
	m.glass_ior = ior; m.ior_base = ior; m.transp_ior = ior;
	m.rg_a2 = alpha * alpha;
	const float fc = 1.f - filt;                                   // filt * filt_col + Rgb(1.f - filt), floats here (:323)
	for(int k = 0; k < 3; ++k) { m.filter_color[k] = filt * fcol[k] + fc; m.mirror_color[k] = scol[k]; }
	m.fake_shadow = fake;
	m.bsdf_flags = 0x2u | 0x10u | 0x20u;                           // BsdfAllGlossy
	if(fake) m.bsdf_flags |= 0x40u;
	if(absorp[0] < 1.f || absorp[1] < 1.f || absorp[2] < 1.f)
	{	// :389-412: vol_i_ = BeerVolumeHandler(absorption, absorption_dist); volumehandler_beer.cc:28-35
		double dist = 1.0;
		p.get("absorption_dist", dist);
		const float maxlog = (float)std::log(1e38);
		for(int k = 0; k < 3; ++k)
		{
			m.beer_sigma[k] = (absorp[k] > 1e-38) ? (float)-std::log((double)absorp[k]) : maxlog;
			if(dist != 0.f) m.beer_sigma[k] = m.beer_sigma[k] * (float)(1.f / dist);
		}
		m.has_vol_i = 1;
		m.bsdf_flags |= 0x100u;                                   // BsdfVolumetric
	}
	return true;
}
// MirrorMaterial::factory + ctor, material_glass.cc:486-493, material_glass.h:74-79
bool make_mirror(const ParamMap &p, yafgpu_material &m)
{
	float col[3] = {1, 1, 1}, refl = 1.f;
	p.getColor("color", col); p.get("reflect", refl);
	std::memset(&m, 0, sizeof m);
	m.type = YAFGPU_MAT_MIRROR; m.receive_shadows = 1;
	for(int k = 0; k < 3; ++k) m.mirror_color[k] = col[k] * refl;
	m.bsdf_flags = 0x1u;
	return true;
}

// AreaLight::factory + ctor, light_area.cc:169-205, :34-52
// Material::isTransparent of the types on this path (yafgpu_shading.h mat_is_transparent)
bool record_is_transparent(const yafgpu_material &m)
{
	return (m.type == YAFGPU_MAT_SHINYDIFFUSE && m.is_transparent) || ((m.type == YAFGPU_MAT_GLASS || m.type == YAFGPU_MAT_ROUGH_GLASS) && m.fake_shadow);
}

// MaskMaterial::factory + ctor, material_mask.cc:133-190, :30-37.  The record's layout: include/yafgpu.h, YAFGPU_MAT_MASKED.
// It reads threshold (a double, kept as a float), material1, material2, receive_shadows, visibility, the node list and `mask` — and
// neither additionaldepth, flat_material, absorption, samplingfactor nor a bump shader.  Where the reference returns nullptr this
// refuses with the cause; a missing `mask`, which leaves the reference a null node to crash on at the first hit, is refused too.
bool make_mask(yafaray_interface *yi, const ParamMap &p, yafaray_material &out)
{
	yafgpu_material &m = out.m;
	double thresh = 0.5; bool recv = true; std::string vis = "normal", name;
	p.get("threshold", thresh);
	const yafaray_material *sub[2] = {nullptr, nullptr};
	for(int k = 0; k < 2; ++k)
	{	// :143-146, :159
		const std::string key = k == 0 ? "material1" : "material2";
		if(!p.get(key, name)) return fail(yi, "mask_mat: " + key + " is missing (material_mask.cc:143-145)");
		auto it = yi->materials.find(name);
		if(it == yi->materials.end()) return fail(yi, "mask_mat: " + key + " \"" + name + "\" names no material defined so far (material_mask.cc:159)");
		if(it->second->m.type == YAFGPU_MAT_MASKED) return fail(yi, "mask_mat: " + key + " \"" + name + "\" is a mask_mat itself: nesting masks is not built on the GPU path");
		if(it->second->m.type == YAFGPU_MAT_BLEND) return fail(yi, "mask_mat: " + key + " \"" + name + "\" is a blend_mat: a blend under a mask (nesting) is not built on the GPU path");
		sub[k] = it->second.get();
	}
	p.get("receive_shadows", recv); p.get("visibility", vis);
	// :165-185: unlike the other node materials, no mask without its nodes
	LoadedNodes ld;
	const int rc = load_nodes(yi, yi->eparams, ld);
	if(rc == 0) return false;
	if(rc < 0) return fail(yi, "mask_mat: the shader node list failed to load (MaskMat: loadNodes() failed, material_mask.cc:180-185)");
	if(!p.get("mask", name)) return fail(yi, "mask_mat: no mask parameter: the reference keeps a null mask node and crashes at the first hit (material_mask.cc:168, :44)");
	auto node = ld.by_name.find(name);
	if(node == ld.by_name.end()) return fail(yi, "mask_mat: mask shader node \"" + name + "\" does not exist (material_mask.cc:172-177)");
	int slot[1] = {node->second};
	if(!sort_nodes(yi, ld, slot, 1, out.nodes)) return false;
	// recursiveRaytrace's glossy branch enters on the CHOSEN material's lobes and picks its case from the mask's flags, the union
	// (integrator_montecarlo.cc:895-919): beside a transmitting partner a glossy sub-material lands in the reflect + transmit case, whose
	// two-direction sample MaskMaterial does not override (Material's default returns black and sends nothing); rough glass, which
	// takes that case alone, finds the same empty default under any mask
	const uint32_t both = sub[0]->m.bsdf_flags | sub[1]->m.bsdf_flags;
	if((both & 0x2u) && (both & 0x10u) && (both & 0x20u))
		return fail(yi, "mask_mat: a glossy sub-material beside one that transmits (or rough glass): recursiveRaytrace reads the union of their flags and takes the "
		                "two-direction sample MaskMaterial does not have (integrator_montecarlo.cc:895-919)");
	std::memset(&m, 0, sizeof m);
	clear_shader_slots(m);
	m.type = YAFGPU_MAT_MASKED; m.visibility = visibility_from(vis); m.receive_shadows = recv;
	m.transmit_filter = (float)thresh;                 // threshold_
	m.bsdf_flags = both;                               // :34
	m.is_transparent = (record_is_transparent(sub[0]->m) || record_is_transparent(sub[1]->m)) ? 1 : 0;      // :86-89
	m.n_nodes = (int32_t)out.nodes.size(); m.sh_diffuse = slot[0];
	m.c_index[0] = m.c_index[1] = -1;                  // the clones' places in the table: flatten_materials
	out.mask_sub[0] = sub[0]->index; out.mask_sub[1] = sub[1]->index;
	return true;
}

// BlendMaterial::factory + ctor, material_blend.cc:464-544, :38-49.  The record's layout: include/yafgpu.h, YAFGPU_MAT_BLEND.
// It reads material1, material2, blend_value (a double, kept as a float), receive_shadows, visibility, mat_pass_index and samplingfactor
// (both read and dropped, as elsewhere), the wireframe parameters (refused unless zero, as for every material), the node list and `mask` —
// and neither additionaldepth (the ctor takes the larger of the sub-materials'), flat_material nor a bump shader.  Where the reference
// returns nullptr this refuses with the cause.  A missing `mask` is no error here: the blend then uses the constant (:518, recalc_blend_
// stays false).  blended_ior_ (:46, getMatIor) is not carried: the integrators read it for ray differentials alone
// (integrator_montecarlo.cc:908, :945, :1013, under diff_rays_enabled_), which the GPU path does not have.
bool make_blend(yafaray_interface *yi, const ParamMap &p, yafaray_material &out)
{
	yafgpu_material &m = out.m;
	double blend_val = 0.5; bool recv = true; std::string vis = "normal", name; float wire = 0.f;
	const yafaray_material *sub[2] = {nullptr, nullptr};
	for(int k = 0; k < 2; ++k)
	{	// :479-482, :501
		const std::string key = k == 0 ? "material1" : "material2";
		if(!p.get(key, name))
			return fail(yi, "blend_mat: " + key + " is missing (material_blend.cc:479-482): a blend of fewer than two materials is outside the GPU path's scope, as it is the "
			                "reference's (createMaterial accepts shinydiffusemat, glossy, coated_glossy, glass, rough_glass, mirror, light_mat, mask_mat, blend_mat)");
		auto it = yi->materials.find(name);
		if(it == yi->materials.end()) return fail(yi, "blend_mat: " + key + " \"" + name + "\" names no material defined so far (material_blend.cc:480-482, :501)");
		if(it->second->m.type == YAFGPU_MAT_MASKED || it->second->m.type == YAFGPU_MAT_BLEND)
			return fail(yi, "blend_mat: " + key + " \"" + name + "\" is a " + (it->second->m.type == YAFGPU_MAT_BLEND ? "blend_mat" : "mask_mat") + " itself: nesting blends and masks is not built on the GPU path");
		if(it->second->m.n_bump > 0)
			return fail(yi, "blend_mat: " + key + " \"" + name + "\" has a bump shader: BlendMaterial::initBsdf blends the two bumped frames (blendSurfacePoints__, surface.cc:137-151), which is not built on the GPU path");
		sub[k] = it->second.get();
	}
	p.get("blend_value", blend_val);
	p.get("receive_shadows", recv); p.get("visibility", vis); p.get("wireframe_amount", wire);
	if(wire != 0.f) return fail(yi, "blend_mat: wireframe shading is not supported by the GPU path");
	// :515-541: the nodes load whether or not `mask` names one
	LoadedNodes ld;
	const int rc = load_nodes(yi, yi->eparams, ld);
	if(rc == 0) return false;
	if(rc < 0) return fail(yi, "blend_mat: the shader node list failed to load (Blend: loadNodes() failed, material_blend.cc:535-540)");
	int slot[1] = {-1};
	out.nodes.clear();
	if(p.get("mask", name))
	{
		auto node = ld.by_name.find(name);
		if(node == ld.by_name.end()) return fail(yi, "blend_mat: mask shader node \"" + name + "\" does not exist (Blend shader node does not exist, material_blend.cc:527-532)");
		slot[0] = node->second;
		if(!sort_nodes(yi, ld, slot, 1, out.nodes)) return false;
	}
	// recursiveRaytrace's glossy branch picks its case from the BLEND's flags, the union (integrator_montecarlo.cc:895-919): a glossy lobe
	// beside a transmitting one takes the reflect + transmit case and BlendMaterial's two-direction sample (material_blend.cc:216-236), which
	// is not restated — the same pairs a mask refuses, in the same words (rough glass has that union alone)
	const uint32_t both = sub[0]->m.bsdf_flags | sub[1]->m.bsdf_flags;
	if((both & 0x2u) && (both & 0x10u) && (both & 0x20u))
		return fail(yi, "blend_mat: a glossy sub-material beside one that transmits (or rough glass): recursiveRaytrace reads the union of their flags and takes the "
		                "two-direction sample, which the GPU path does not have for a blend (integrator_montecarlo.cc:895-919)");
	std::memset(&m, 0, sizeof m);
	clear_shader_slots(m);
	m.type = YAFGPU_MAT_BLEND; m.visibility = visibility_from(vis); m.receive_shadows = recv;
	m.transmit_filter = (float)blend_val;              // blend_val_ (:45)
	m.bsdf_flags = both;                               // :42
	m.additional_depth = std::max(sub[0]->m.additional_depth, sub[1]->m.additional_depth);      // :48
	m.is_transparent = (record_is_transparent(sub[0]->m) || record_is_transparent(sub[1]->m)) ? 1 : 0;      // :332-335
	m.n_nodes = (int32_t)out.nodes.size(); m.sh_diffuse = slot[0];      // (sort_nodes left the node's place among them)
	{	// getVolumeHandler, :450-462 (inside: the only handler a material on this path has is glass's vol_i_); by the CONSTANT blend_val_
		const yafgpu_material *v1 = sub[0]->m.has_vol_i ? &sub[0]->m : nullptr, *v2 = sub[1]->m.has_vol_i ? &sub[1]->m : nullptr;
		const yafgpu_material *v = (v1 && v2) ? (m.transmit_filter <= 0.5f ? v1 : v2) : (v1 ? v1 : v2);
		if(v) { m.has_vol_i = 1; for(int k = 0; k < 3; ++k) m.beer_sigma[k] = v->beer_sigma[k]; }
	}
	m.c_index[0] = m.c_index[1] = -1;                  // the clones' places in the table: flatten_materials
	out.mask_sub[0] = sub[0]->index; out.mask_sub[1] = sub[1]->index;
	return true;
}

// The material table of the device scene: the materials in creation order, then, for every mask_mat, a clone of each of its two
// sub-materials, which is what a vertex on the mask gets (yafgpu_wavefront.h wf_mask_hit).  A clone is the sub-material with the
// material-level values the integrators read off sp.material_, the MASK, in the reference: receive_shadows (integrator_montecarlo.cc:91)
// and visibility are the mask's; isFlat() (:105, :189) is false, while ShinyDiffuseMaterial::eval's own flat_material_ test
// (material_shiny_diffuse.cc:275) stays the sub-material's (flat 2); getAdditionalDepth() (integrator_path_tracer.cc:149) and the
// transparent bias (integrator_montecarlo.cc:1003-1011) are 0; getVolumeHandler() (:912, :991, integrator_path_tracer.cc:276) is null,
// so glass under a mask does not absorb.  Its nodes are the sub-material's own range, shared.
void flatten_materials(const yafaray_interface *yi, std::vector<yafgpu_material> &mats, std::vector<yafgpu_node> &nodes)
{
	mats.clear(); nodes.clear();
	for(auto *m : yi->material_order)
	{
		yafgpu_material rec = m->m;
		rec.node_first = (int32_t)nodes.size();           // rec.n_nodes colour nodes, then the bump shader's list
		rec.bump_first += rec.node_first;
		nodes.insert(nodes.end(), m->nodes.begin(), m->nodes.end());
		mats.push_back(rec);
	}
	const size_t n = mats.size();
	for(size_t i = 0; i < n; ++i)
	{
		if(mats[i].type == YAFGPU_MAT_BLEND)
		{	// a blend_mat's clones, in the same place: the two records its functions run on (yafgpu_shading.h BlendScratch).  The vertex's
			// material stays the blend, so no material-level word of a clone is ever read; each is the sub-material as it is, nodes shared,
			// but for flat: isFlat() is the blend's (false), ShinyDiffuseMaterial::eval's own test stays (2)
			for(int k = 0; k < 2; ++k)
			{
				yafgpu_material c = mats[(size_t)yi->material_order[i]->mask_sub[k]];
				c.flat = c.flat ? 2 : 0;
				mats[i].c_index[k] = (int32_t)mats.size();
				mats.push_back(c);
			}
			continue;
		}
		if(mats[i].type != YAFGPU_MAT_MASKED) continue;
		for(int k = 0; k < 2; ++k)
		{
			yafgpu_material c = mats[(size_t)yi->material_order[i]->mask_sub[k]];
			c.receive_shadows = mats[i].receive_shadows; c.visibility = mats[i].visibility;
			c.flat = c.flat ? 2 : 0;
			c.additional_depth = 0; c.transp_bias_factor = 0.f; c.transp_bias_mult = 0;
			c.has_vol_i = 0; c.beer_sigma[0] = c.beer_sigma[1] = c.beer_sigma[2] = 0.f;
			mats[i].c_index[k] = (int32_t)mats.size();
			mats.push_back(c);
		}
	}
}

bool make_arealight(const ParamMap &p, yafgpu_light &l)
{
	float corner[3] = {0, 0, 0}, p1[3] = {0, 0, 0}, p2[3] = {0, 0, 0}, color[3] = {1, 1, 1};
	float power = 1.f; int samples = 4; bool enabled = true, cast = true;
	p.getPoint("corner", corner); p.getPoint("point1", p1); p.getPoint("point2", p2); p.getColor("color", color);
	p.get("power", power); p.get("samples", samples); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_AREA; l.samples = samples; l.cast_shadows = cast;
	float tx[3], ty[3];
	for(int k = 0; k < 3; ++k) { l.corner[k] = corner[k]; tx[k] = p1[k] - corner[k]; ty[k] = p2[k] - corner[k]; l.to_x[k] = tx[k]; l.to_y[k] = ty[k]; }
	float fn[3]; cross3(ty, tx, fn);
	for(int k = 0; k < 3; ++k) l.color[k] = (power * color[k]) * (float)kPi;   // col * inte * M_PI
	float vl = fn[0] * fn[0] + fn[1] * fn[1] + fn[2] * fn[2];                 // normLen, vector.h:61-71
	if(vl != 0.f) { vl = std::sqrt(vl); const float d = (float)(1.0 / (double)vl); fn[0] *= d; fn[1] *= d; fn[2] *= d; }
	l.area = vl;
	for(int k = 0; k < 3; ++k)
	{
		l.fnormal[k] = fn[k];
		l.c2[k] = corner[k] + tx[k];
		l.c3[k] = corner[k] + (tx[k] + ty[k]);
		l.c4[k] = corner[k] + ty[k];
	}
	return enabled;
}
// PointLight::factory + ctor, light_point.cc:97-120, :28-36
bool make_pointlight(const ParamMap &p, yafgpu_light &l)
{
	float from[3] = {0, 0, 0}, color[3] = {1, 1, 1}; float power = 1.f; bool enabled = true, cast = true;
	p.getPoint("from", from); p.getColor("color", color); p.get("power", power); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_POINT; l.samples = 1; l.cast_shadows = cast;
	for(int k = 0; k < 3; ++k) { l.position[k] = from[k]; l.color[k] = power * color[k]; }
	return enabled;
}

inline float host_fsin_poly(float x)   // fSin__ with FAST_TRIG, util_math_optimizations.h:219-244
{
	const double k2Pi = 6.28318530717958647692, kPi = 3.14159265358979323846;
	if((double)x > k2Pi || (double)x < -k2Pi) x -= ((int)(x * (float)0.15915494309189533577)) * (float)k2Pi;
	if((double)x < -kPi) x += (float)k2Pi;
	else if((double)x > kPi) x -= (float)k2Pi;
	x = ((float)1.27323954473516268615 * x) - ((float)0.40528473456935108578 * x * std::fabs(x));
	const float result = 0.225f * (x * std::fabs(x) - x) + x;
	if(result <= -1.0f) return -1.0f;
	if(result >= 1.0f) return 1.0f;
	return result;
}
// Vec3::normalize, vector.h (len = 1.0 / fSqrt__(len) in double, narrowed)
inline void ref_normalize(float *v)
{
	float len = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
	if(len != 0.f) { len = (float)(1.0 / (double)std::sqrt(len)); v[0] *= len; v[1] *= len; v[2] *= len; }
}
// createCs__, vector.h:319-337
inline void ref_create_cs(const float *n, float *u, float *v)
{
	if(n[0] == 0.f && n[1] == 0.f)
	{
		u[0] = n[2] < 0.f ? -1.f : 1.f; u[1] = 0.f; u[2] = 0.f;
		v[0] = 0.f; v[1] = 1.f; v[2] = 0.f;
	}
	else
	{
		const float d = (float)(1.0 / (double)std::sqrt(n[1] * n[1] + n[0] * n[0]));
		u[0] = n[1] * d; u[1] = -n[0] * d; u[2] = 0.f;
		cross3(n, u, v);
	}
}
// with_caustic / with_diffuse: photon-mapping settings, read by the reference's factories and dropped here (photon_only is refused by the caller)
// DirectionalLight::factory + ctor, light_directional.cc:118-158, :31-42: `from` (or the deprecated `position`) and `radius` are only read
// for a finite light; an infinite one's shadow rays have no end (illuminate, :60-80)
bool make_directionallight(const ParamMap &p, yafgpu_light &l)
{
	float from[3] = {0, 0, 0}, dir[3] = {0, 0, 1}, color[3] = {1, 1, 1};
	float power = 1.f, rad = 1.f; bool inf = true, enabled = true, cast = true;
	p.getPoint("direction", dir); p.getColor("color", color); p.get("power", power); p.get("infinite", inf);
	p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	if(!inf)
	{
		if(!p.getPoint("from", from)) p.getPoint("position", from);
		p.get("radius", rad);
	}
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_DIRECTIONAL; l.samples = 1; l.cast_shadows = cast; l.infinite = inf;
	for(int k = 0; k < 3; ++k) { l.position[k] = from[k]; l.direction[k] = dir[k]; l.color[k] = color[k] * power; }
	ref_normalize(l.direction);
	ref_create_cs(l.direction, l.du, l.dv);
	l.radius = rad;
	return enabled;
}
// SunLight::factory + ctor, light_sun.cc:96-125, :29-42
bool make_sunlight(const ParamMap &p, yafgpu_light &l)
{
	float dir[3] = {0, 0, 1}, color[3] = {1, 1, 1};
	float power = 1.f, angle = 0.27f; int samples = 4; bool enabled = true, cast = true;
	p.getPoint("direction", dir); p.getColor("color", color); p.get("power", power); p.get("angle", angle); p.get("samples", samples);
	p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_SUN; l.samples = samples; l.cast_shadows = cast;
	for(int k = 0; k < 3; ++k) { l.direction[k] = dir[k]; l.color[k] = color[k] * power; }
	ref_normalize(l.direction);
	ref_create_cs(dir, l.du, l.dv);                 // createCs__(dir, ...): the direction as given, not the normalised one (:36)
	if(angle > 80.f) angle = 80.f;
	l.cos_angle = host_fsin_poly((float)((double)angle * 0.01745329251994329576922) + (float)1.57079632679489661923);   // fCos__(DEG_TO_RAD(angle))
	l.invpdf = (float)(6.28318530717958647692 * (double)(1.f - l.cos_angle));                                           // M_2PI * (1 - cos_angle_)
	l.pdf = (float)(1.0 / (double)l.invpdf);
	for(int k = 0; k < 3; ++k) l.col_pdf[k] = l.color[k] * l.pdf;
	return enabled;
}
// SphereLight::factory + ctor, light_sphere.cc:165-195, :31-41.  `object` names the mesh the exporter pairs with the light; SphereLight::init
// (:45-55) only hands that mesh a pointer to the light, for photon mapping.  Here the mesh stays the ordinary (light-material) geometry it is.
bool make_spherelight(const ParamMap &p, yafgpu_light &l)
{
	float from[3] = {0, 0, 0}, color[3] = {1, 1, 1};
	float power = 1.f, radius = 1.f; int samples = 4, object = 0; bool enabled = true, cast = true;
	p.getPoint("from", from); p.getColor("color", color); p.get("power", power); p.get("radius", radius); p.get("samples", samples);
	p.get("object", object); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	(void)object;
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_SPHERE; l.samples = samples; l.cast_shadows = cast;
	for(int k = 0; k < 3; ++k) { l.position[k] = from[k]; l.color[k] = color[k] * power; }
	l.radius = radius;
	l.square_radius = radius * radius;
	l.square_radius_epsilon = (float)((double)l.square_radius * 1.000003815);    // ~0.2 % larger radius squared
	return enabled;
}
// MeshLight::factory + ctor, light_meshlight.cc:231-262, :34-43.  The mesh is looked up when the scene is made (MeshLight::init, :75-86;
// flatten_scene here): until then the record names no rows (mesh_first -1) and has no area
bool make_meshlight(const ParamMap &p, yafgpu_light &l, unsigned int &object_id)
{
	float color[3] = {1, 1, 1};
	double power = 1.0; int samples = 4, object = 0; bool double_s = false, enabled = true, cast = true;
	p.get("object", object); p.getColor("color", color); p.get("power", power); p.get("samples", samples); p.get("double_sided", double_s);
	p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_MESH; l.samples = samples; l.cast_shadows = cast; l.double_sided = double_s;
	l.mesh_first = -1;
	for(int k = 0; k < 3; ++k) l.color[k] = (color[k] * (float)power) * (float)kPi;   // color * (float)power * M_PI (:255): Rgb * float twice (color.h:266 narrows M_PI)
	object_id = (unsigned int)object;
	return enabled;
}
// BackgroundPortalLight::factory + ctor, light_background_portal.cc:237-264, :34-43.  power is a float here (:241); no color and no
// double_sided.  The mesh is looked up when the scene is made (init, :79-96; flatten_scene here): until then the record has no
// triangles (mesh_pool -1) and no area.  clamp_intersect stays 0: only the background's own factory sets it, on its own light
bool make_portallight(const ParamMap &p, yafgpu_light &l, unsigned int &object_id)
{
	float power = 1.0f; int samples = 4, object = 0; bool enabled = true, cast = true;
	p.get("object", object); p.get("samples", samples); p.get("power", power); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	std::memset(&l, 0, sizeof l);
	l.type = YAFGPU_LIGHT_PORTAL; l.samples = samples; l.cast_shadows = cast;
	l.mesh_first = -1; l.mesh_pool = -1;
	l.portal_power = power;
	object_id = (unsigned int)object;
	return enabled;
}
// IesLight::factory + ctor, light_ies.cc:190-233, :30-49.  cone_angle is read and unused, as there; tot_energy_ serves photon emission only.
// ies_first is filled when the scene is made (flatten_scene), where the lights' tables meet in one pool.
// Returns whether the light was made; `enabled` is then light_enabled.
bool make_ieslight(yafaray_interface *yi, const ParamMap &p, yafgpu_light &l, yafies::Data &ies, bool &enabled)
{
	float from[3] = {0, 0, 0}, to[3] = {0, 0, -1}, color[3] = {1, 1, 1};
	float power = 1.f, ang = 180.f; int samples = 16; bool soft = false, cast = true;
	std::string file;
	enabled = true;
	p.getPoint("from", from); p.getPoint("to", to); p.getColor("color", color); p.get("power", power); p.get("file", file); p.get("samples", samples);
	p.get("soft_shadows", soft); p.get("cone_angle", ang); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	(void)ang;
	std::string err, path = file;
	{	// the name as given first, then beside the XML file, as createTexture resolves `filename`
		FILE *f = std::fopen(path.c_str(), "rb");
		if(f) std::fclose(f);
		else if(!yi->base_dir.empty() && !file.empty() && file[0] != '/') path = yi->base_dir + "/" + file;
	}
	if(!yafies::parse_file(path, ies, err)) { fail(yi, "createLight: " + err); return false; }
	std::memset(&l, 0, sizeof l);
	l.type = soft ? YAFGPU_LIGHT_IES_SOFT : YAFGPU_LIGHT_IES; l.samples = soft ? samples : 1; l.cast_shadows = cast;
	float dir[3];
	for(int k = 0; k < 3; ++k) { l.position[k] = from[k]; l.direction[k] = from[k] - to[k]; l.color[k] = color[k] * power; }
	ref_normalize(l.direction);
	for(int k = 0; k < 3; ++k) dir[k] = -l.direction[k];
	ref_create_cs(dir, l.du, l.dv);
	l.cos_angle = host_fsin_poly(ies.max_v_angle + (float)1.57079632679489661923);      // fCos__(getMaxVAngle())
	l.ies_first = -1; l.ies_n_hor = ies.n_hor; l.ies_n_vert = ies.n_vert; l.ies_type = ies.type; l.ies_max_rad = ies.max_rad;
	return true;
}
// SpotLight::factory + ctor, light_spot.cc:258-296, :29-42.  The Pdf1D of the smoothstep and interv_1_ / interv_2_ (:44-68) serve photon
// emission only; with_caustic and with_diffuse are read by the factory and dropped here.  The caller has made sure that `from` and `to` are
// both there.  Returns whether the light was made; `enabled` is then light_enabled.
bool make_spotlight(yafaray_interface *yi, const ParamMap &p, yafgpu_light &l, bool &enabled)
{
	float from[3] = {0, 0, 0}, to[3] = {0, 0, -1}, color[3] = {1, 1, 1};
	float power = 1.f, angle = 45.f, falloff = 0.15f, ssfuzzy = 1.f; int samples = 8; bool soft = false, cast = true;
	enabled = true;
	p.getPoint("from", from); p.getPoint("to", to); p.getColor("color", color); p.get("power", power); p.get("cone_angle", angle); p.get("blend", falloff);
	p.get("soft_shadows", soft); p.get("shadowFuzzyness", ssfuzzy); p.get("samples", samples); p.get("light_enabled", enabled); p.get("cast_shadows", cast);
	if(from[0] == to[0] && from[1] == to[1] && from[2] == to[2]) { fail(yi, "createLight: spotlight: from and to are the same point, the light has no axis"); return false; }
	if(!(std::isfinite(angle) && angle > 0.f && angle <= 180.f)) { fail(yi, "createLight: spotlight: cone_angle must lie in (0, 180]"); return false; }
	if(!(std::isfinite(falloff) && falloff >= 0.f && falloff <= 1.f)) { fail(yi, "createLight: spotlight: blend must lie in [0, 1]"); return false; }
	if(soft && samples < 1) { fail(yi, "createLight: spotlight: samples must be at least 1 with soft_shadows"); return false; }
	std::memset(&l, 0, sizeof l);
	l.type = soft ? YAFGPU_LIGHT_SPOT_SOFT : YAFGPU_LIGHT_SPOT; l.samples = soft ? samples : 1; l.cast_shadows = cast;
	float dir[3];
	for(int k = 0; k < 3; ++k) { l.position[k] = from[k]; l.direction[k] = from[k] - to[k]; l.color[k] = color[k] * power; }
	ref_normalize(l.direction);                           // ndir_
	for(int k = 0; k < 3; ++k) dir[k] = -l.direction[k];  // dir_
	ref_create_cs(dir, l.du, l.dv);
	const double rad_angle = (double)angle * 0.01745329251994329576922;      // DEG_TO_RAD(angle)
	const double rad_inner_angle = rad_angle * (double)(1.f - falloff);
	l.spot_cos_start = host_fsin_poly((float)rad_inner_angle + (float)1.57079632679489661923);      // fCos__ narrows its argument
	l.cos_angle = host_fsin_poly((float)rad_angle + (float)1.57079632679489661923);                 // cos_end_
	l.spot_icos_diff = (float)(1.0 / (double)(l.spot_cos_start - l.cos_angle));                     // infinite with blend 0: never read then
	l.spot_shadow_fuzzy = ssfuzzy;
	return true;
}

// PerspectiveCamera::factory, Camera::Camera, setAxis — camera_perspective.cc:198-243, camera.cc:46-66, :60-74
bool make_camera(yafaray_interface *yi, const ParamMap &p, yafgpu_camera &c)
{
	float from[3] = {0, 1, 0}, to[3] = {0, 0, 0}, up[3] = {0, 1, 1};
	int resx = 320, resy = 200; float aspect = 1, dfocal = 1, apt = 0, near_clip = 0.f, far_clip = -1.f;
	p.getPoint("from", from); p.getPoint("to", to); p.getPoint("up", up); p.get("resx", resx); p.get("resy", resy);
	p.get("focal", dfocal); p.get("aperture", apt); p.get("aspect_ratio", aspect); p.get("nearClip", near_clip); p.get("farClip", far_clip);
	float dofd = 0.f, bkhrot = 0.f; std::string bkhtype = "disk1", bkhbias = "uniform";
	p.get("dof_distance", dofd); p.get("bokeh_type", bkhtype); p.get("bokeh_bias", bkhbias); p.get("bokeh_rotation", bkhrot);
	(void)yi;
	const float aspect_ratio = aspect * (float)resy / (float)resx;
	float cy[3], cz[3], cx[3];
	for(int k = 0; k < 3; ++k) { cy[k] = up[k] - from[k]; cz[k] = to[k] - from[k]; }
	cross3(cz, cy, cx);
	cross3(cz, cx, cy);
	normalize3(cx); normalize3(cy); normalize3(cz);
	std::memset(&c, 0, sizeof c);
	c.resx = resx; c.resy = resy;
	for(int k = 0; k < 3; ++k)
	{
		c.position[k] = from[k];
		c.near_n[k] = cz[k]; c.near_p[k] = from[k] + near_clip * cz[k];
		c.far_n[k] = cz[k]; c.far_p[k] = from[k] + far_clip * cz[k];
		const float vright = cx[k], vup = aspect_ratio * cy[k];
		c.vto[k] = (dfocal * cz[k]) - 0.5f * (vup + vright);
		c.vup[k] = vup / (float)resy;
		c.vright[k] = vright / (float)resx;
		c.dof_rt[k] = apt * cx[k]; c.dof_up[k] = apt * cy[k];         // setAxis, :66-67
		c.cam_x[k] = cx[k]; c.cam_y[k] = cy[k]; c.cam_z[k] = cz[k];
	}
	c.focal_distance = dfocal; c.aspect_ratio = aspect_ratio;
	c.aperture = apt; c.dof_distance = dofd; c.bokeh_rotation = bkhrot;
	c.bokeh_type = bkhtype == "disk2" ? 1 : bkhtype == "triangle" ? 3 : bkhtype == "square" ? 4 : bkhtype == "pentagon" ? 5
	             : bkhtype == "hexagon" ? 6 : bkhtype == "ring" ? 7 : 0;
	c.bokeh_bias = bkhbias == "center" ? 1 : bkhbias == "edge" ? 2 : 0;
	return true;
}
// ArchitectCamera::factory, ctor, setAxis — camera_architect.cc:92-133, :29-50, :52-66.  The factory's parameters and defaults are
// PerspectiveCamera's (farClip -1 included) and the ctor runs PerspectiveCamera's first, so the record starts as make_camera's; then the
// class's own setAxis replaces vup_ by aspect_ratio_ * Vec3(0, 0, -1) — verticals stay vertical — and rebuilds vto_ from it.  dof_rt_ /
// dof_up_ still follow cam_x_ / cam_y_ (:58-59) and the corner table is filled again with the same values (:37-49).  The rays are
// PerspectiveCamera::shootRay's (the class does not override it): nothing differs on the device but screenproject.
bool make_architect_camera(yafaray_interface *yi, const ParamMap &p, yafgpu_camera &c)
{
	if(!make_camera(yi, p, c)) return false;
	c.type = YAFGPU_CAMERA_ARCHITECT;
	const float up_axis[3] = {0.f, 0.f, -1.f};
	for(int k = 0; k < 3; ++k)
	{
		const float vright = c.cam_x[k], vup = c.aspect_ratio * up_axis[k];
		c.vto[k] = (c.cam_z[k] * c.focal_distance) - 0.5f * (vup + vright);
		c.vup[k] = vup / (float)c.resy;
	}
	return true;
}
// AngularCamera::factory + ctor + setAxis (camera_angular.cc:82-121, :29-53) and EquirectangularCamera's (camera_equirectangular.cc:67-90,
// :29-47) over Camera::Camera (camera.cc:46-66).  vright_ / vup_ / vto_ are the unit axes.  Neither class overrides Camera::sampleLense()
// (camera.h: false), so the integrator never draws lens samples for them: `aperture` stays 0 in the record whatever the ParamMap carries —
// the device keys the lens stream on it (wf_generate) — and so do the other depth-of-field fields.
// The unqualified tan() of the ctor (:38, :40) is the double C function, its result narrowed into focal_length_; fSin__ is the float polynomial.
bool make_panoramic_camera(yafaray_interface *yi, const ParamMap &p, bool angular, yafgpu_camera &c)
{
	float from[3] = {0, 1, 0}, to[3] = {0, 0, 0}, up[3] = {0, 1, 1};
	int resx = 320, resy = 200;
	double aspect_d = 1.0, angle_degrees = 90, max_angle_degrees = 90;
	std::string projection_string;
	bool circular = true, mirrored = false;
	float near_clip = 0.0f, far_clip = -1.0e38f;
	p.getPoint("from", from); p.getPoint("to", to); p.getPoint("up", up); p.get("resx", resx); p.get("resy", resy);
	p.get("aspect_ratio", aspect_d);
	if(angular)
	{
		p.get("angle", angle_degrees);
		max_angle_degrees = angle_degrees;
		p.get("max_angle", max_angle_degrees);
		p.get("circular", circular); p.get("mirrored", mirrored); p.get("projection", projection_string);
	}
	p.get("nearClip", near_clip); p.get("farClip", far_clip);
	const float aspect = (float)aspect_d;
	const float aspect_ratio = aspect * (float)resy / (float)resx;
	float cy[3], cz[3], cx[3];
	for(int k = 0; k < 3; ++k) { cy[k] = up[k] - from[k]; cz[k] = to[k] - from[k]; }
	cross3(cz, cy, cx);
	cross3(cz, cx, cy);
	normalize3(cx); normalize3(cy); normalize3(cz);
	std::memset(&c, 0, sizeof c);
	c.type = angular ? YAFGPU_CAMERA_ANGULAR : YAFGPU_CAMERA_EQUIRECTANGULAR;
	c.resx = resx; c.resy = resy;
	for(int k = 0; k < 3; ++k)
	{
		c.position[k] = from[k];
		c.near_n[k] = cz[k]; c.near_p[k] = from[k] + cz[k] * near_clip;
		c.far_n[k] = cz[k]; c.far_p[k] = from[k] + cz[k] * far_clip;
		c.vright[k] = cx[k]; c.vup[k] = cy[k]; c.vto[k] = cz[k];
		c.cam_x[k] = cx[k]; c.cam_y[k] = cy[k]; c.cam_z[k] = cz[k];
	}
	c.aspect_ratio = aspect_ratio;
	if(!angular) return true;
	if(!(angle_degrees > 0.0)) return fail(yi, "createCamera: angular camera: angle must be above 0 degrees");
	const float angle = (float)(angle_degrees * 3.14159265358979323846 / (double)180.f), max_angle = (float)(max_angle_degrees * 3.14159265358979323846 / (double)180.f);
	c.max_radius = max_angle / angle;
	c.circular = circular ? 1 : 0;
	c.projection = projection_string == "orthographic" ? YAFGPU_ANGULAR_ORTHOGRAPHIC : projection_string == "stereographic" ? YAFGPU_ANGULAR_STEREOGRAPHIC
	             : projection_string == "equisolid_angle" ? YAFGPU_ANGULAR_EQUISOLID_ANGLE : projection_string == "rectilinear" ? YAFGPU_ANGULAR_RECTILINEAR
	             : YAFGPU_ANGULAR_EQUIDISTANT;
	if(c.projection == YAFGPU_ANGULAR_ORTHOGRAPHIC) c.focal_length = 1.f / host_fsin_poly(angle);
	else if(c.projection == YAFGPU_ANGULAR_STEREOGRAPHIC) c.focal_length = (float)((double)(1.f / 2.f) / std::tan((double)(angle / 2.f)));
	else if(c.projection == YAFGPU_ANGULAR_EQUISOLID_ANGLE) c.focal_length = 1.f / 2.f / host_fsin_poly(angle / 2.f);
	else if(c.projection == YAFGPU_ANGULAR_RECTILINEAR) c.focal_length = (float)((double)1.f / std::tan((double)angle));
	else c.focal_length = 1.f / angle;
	if(mirrored) for(int k = 0; k < 3; ++k) c.vright[k] *= -1.0f;      // :116, after the ctor: cam_x_ (screenproject) keeps its sign
	if(c.projection == YAFGPU_ANGULAR_ORTHOGRAPHIC || c.projection == YAFGPU_ANGULAR_EQUISOLID_ANGLE)
	{	// shootRay :68 / :70 takes asin(radius / focal_length_) resp. asin(radius / (2 focal_length_)): above 1 the reference hands the integrator
		// a NaN direction.  Such a camera is refused here instead.  The largest radius a sample reaches is the frame's corner, or the circle's.
		float radius = std::sqrt(1.f + aspect_ratio * aspect_ratio);
		if(circular && c.max_radius < radius) radius = c.max_radius;
		const float arg = c.projection == YAFGPU_ANGULAR_ORTHOGRAPHIC ? radius / c.focal_length : radius / (2.f * c.focal_length);
		if(!(arg <= 1.f))
			return fail(yi, "createCamera: angular camera: projection \"" + projection_string + "\" reaches past its domain with this angle / max_angle"
			            " (asin of " + std::to_string(arg) + " at the largest radius " + std::to_string(radius) + "): use circular with a smaller max_angle, or a smaller angle");
	}
	return true;
}

void set_param(yafaray_interface *yi, const char *name, const Param &v) { if(name) yi->cparams->dicc[name] = v; }

} // namespace

extern "C" {

yafaray_interface_t *yafaray_createInterface(void) { return new yafaray_interface(); }
void yafaray_destroyInterface(yafaray_interface_t *yi)
{
	if(!yi) return;
	if(yi->gpu) yafgpu_scene_destroy(yi->gpu);
	delete yi;
}
const char *yafaray_getLastError(const yafaray_interface_t *yi) { return yi ? yi->err.c_str() : "null interface"; }
const char *yafaray_getVersion(void) { return "yafgpu-0.1 (MI355X path-tracing core behind the libYafaRay v3 Interface API)"; }

yafaray_bool_t yafaray_startScene(yafaray_interface_t *yi, int type)
{
	if(type != 0) return fail(yi, "startScene: only scene type 0 (\"triangle\") is supported (import_xml.cc:339-347)");
	yi->state = 0; yi->meshes.clear(); yi->instances.clear(); yi->curves.clear(); yi->cur = nullptr; yi->last = nullptr; yi->cur_curve = nullptr; yi->last_is_curve = false; yi->geometry_changed = true; yi->prepared = false; yi->scene_dirty = true;
	return 1;
}
yafaray_bool_t yafaray_startGeometry(yafaray_interface_t *yi) { if(yi->state != 0) return fail(yi, "startGeometry: wrong state"); yi->state = 1; return 1; }
yafaray_bool_t yafaray_endGeometry(yafaray_interface_t *yi) { if(yi->state != 1) return fail(yi, "endGeometry: wrong state"); yi->state = 0; return 1; }
unsigned int yafaray_getNextFreeId(yafaray_interface_t *yi) { while(yi->meshes.count(yi->next_id) || yi->instances.count(yi->next_id) || yi->curves.count(yi->next_id)) ++yi->next_id; return yi->next_id++; }

// Between startCurveMesh and endCurveMesh only addVertex means something (import_xml.cc:504-509): the reference would push whatever else
// comes into the TriangleObject that endCurveMesh then indexes by point count.  Refused with the cause.
static bool in_curve(yafaray_interface_t *yi, const char *call)
{
	if(yi->state != 3) return false;
	fail(yi, std::string(call) + ": a curve mesh is open (startCurveMesh): between it and endCurveMesh only addVertex is accepted");
	return true;
}

yafaray_bool_t yafaray_startTriMesh(yafaray_interface_t *yi, unsigned int id, int vertices, int triangles, yafaray_bool_t has_orco, yafaray_bool_t has_uv, int type, int)
{
	if(in_curve(yi, "startTriMesh")) return 0;
	if(yi->state != 1) return fail(yi, "startTriMesh: wrong state");
	if((type & 0xFF) != 0) return fail(yi, "startTriMesh: only TRIM meshes (type 0) are supported");
	note_srand(yi, ++g_object_index_auto);          // ObjectGeometric::ObjectGeometric, object_geom.cc:39-43
	yi->instances.erase(id);                        // meshes_[id] is one slot: a mesh started under an instance's id takes its place
	yi->curves.erase(id); yi->last_is_curve = false;
	Mesh &m = yi->meshes[id];
	m = Mesh();
	m.visible = !(type & 0x0100); m.base = (type & 0x0200) != 0;
	m.has_orco = has_orco != 0; m.has_uv = has_uv != 0;
	m.points.reserve((size_t)std::max(vertices, 0) * 3); m.tri.reserve((size_t)std::max(triangles, 0) * 3); m.tri_mat.reserve((size_t)std::max(triangles, 0));
	yi->cur = &m; yi->last = &m; yi->state = 2; yi->geometry_changed = true; yi->prepared = false; yi->scene_dirty = true;
	return 1;
}
yafaray_bool_t yafaray_endTriMesh(yafaray_interface_t *yi)
{	// Scene::endTriMesh, scene.cc:311-337: "UV-offsets mismatch!" when the triangle and UV-offset counts disagree; the reference never
	// range-checks the offsets themselves (exporters may list <uv> after the faces), so that check waits until here
	if(in_curve(yi, "endTriMesh")) return 0;
	if(yi->state != 2) return fail(yi, "endTriMesh: wrong state");
	Mesh &m = *yi->cur;
	if(m.has_uv)
	{
		if(m.tri_uv.size() != m.tri.size()) return fail(yi, "endTriMesh: UV-offsets mismatch!");
		const int nuv = (int)(m.uv.size() / 2);
		for(int o : m.tri_uv) if(o < 0 || o >= nuv) return fail(yi, "endTriMesh: UV index out of range");
	}
	yi->state = 1; yi->cur = nullptr;
	return 1;
}
int yafaray_addVertex(yafaray_interface_t *yi, double x, double y, double z)
{
	if(yi->state == 3)
	{	// a point of the open curve's poly-line (startElCurve__, import_xml.cc:504-509)
		Curve &c = *yi->cur_curve;
		c.points.push_back((float)x); c.points.push_back((float)y); c.points.push_back((float)z);
		return (int)(c.points.size() / 3) - 1;
	}
	if(yi->state != 2) { fail(yi, "addVertex: wrong state"); return -1; }
	Mesh &m = *yi->cur;
	m.points.push_back((float)x); m.points.push_back((float)y); m.points.push_back((float)z);
	return (int)(m.points.size() / 3) - 1;
}
void yafaray_addNormal(yafaray_interface_t *yi, double nx, double ny, double nz)
{	// Scene::addNormal, scene.cc:592-607: attaches to the last vertex
	if(in_curve(yi, "addNormal")) return;
	if(yi->state != 2) { fail(yi, "addNormal: wrong state"); return; }
	Mesh &m = *yi->cur;
	const size_t nv = m.points.size() / 3;
	if(nv == 0) return;
	if(m.normals.size() < nv * 3) m.normals.resize(nv * 3, 0.f);
	m.normals[(nv - 1) * 3] = (float)nx; m.normals[(nv - 1) * 3 + 1] = (float)ny; m.normals[(nv - 1) * 3 + 2] = (float)nz;
	m.normals_exported = true;
}
yafaray_bool_t yafaray_addTriangle(yafaray_interface_t *yi, int a, int b, int c, const yafaray_material_t *mat)
{
	if(in_curve(yi, "addTriangle")) return 0;
	if(yi->state != 2) return fail(yi, "addTriangle: wrong state");
	if(!mat) return fail(yi, "addTriangle: null material");
	Mesh &m = *yi->cur;
	const int nv = (int)(m.points.size() / 3);
	if(a < 0 || b < 0 || c < 0 || a >= nv || b >= nv || c >= nv) return fail(yi, "addTriangle: vertex index out of range");
	m.tri.push_back(a); m.tri.push_back(b); m.tri.push_back(c); m.tri_mat.push_back(mat->index);
	return 1;
}
int yafaray_addVertexWithOrco(yafaray_interface_t *yi, double x, double y, double z, double ox, double oy, double oz)
{	// Interface::addVertex(x, y, z, ox, oy, oz) -> Scene::addVertex(p, orco), scene.cc:567-590
	if(in_curve(yi, "addVertex")) return -1;        // state_.orco_ is false in a curve (scene.cc:147)
	if(yi->state != 2) { fail(yi, "addVertex: wrong state"); return -1; }
	Mesh &m = *yi->cur;
	if(!m.has_orco) { fail(yi, "addVertex: the mesh was started without orco coordinates"); return -1; }
	m.points.push_back((float)x); m.points.push_back((float)y); m.points.push_back((float)z);
	m.orco.resize(m.points.size(), 0.f);
	const size_t k = m.points.size() - 3;
	m.orco[k] = (float)ox; m.orco[k + 1] = (float)oy; m.orco[k + 2] = (float)oz;
	return (int)(m.points.size() / 3) - 1;
}
int yafaray_addUv(yafaray_interface_t *yi, float u, float v)
{	// Scene::addUv, scene.cc:672-686
	if(in_curve(yi, "addUv")) return -1;
	if(yi->state != 2 || !yi->cur) { fail(yi, "addUv: wrong state"); return -1; }
	Mesh &m = *yi->cur;
	m.uv.push_back(u); m.uv.push_back(v);
	return (int)(m.uv.size() / 2) - 1;
}
yafaray_bool_t yafaray_addTriangleWithUv(yafaray_interface_t *yi, int a, int b, int c, int uv_a, int uv_b, int uv_c, const yafaray_material_t *mat)
{	// Interface::addTriangle(a, b, c, uv_a, uv_b, uv_c, mat) -> Scene::addTriangle, scene.cc:652-670
	if(in_curve(yi, "addTriangle")) return 0;
	if(yi->state != 2) return fail(yi, "addTriangle: wrong state");
	Mesh &m = *yi->cur;
	if(!m.has_uv) return fail(yi, "addTriangle: the mesh was started without UV coordinates");
	if(!yafaray_addTriangle(yi, a, b, c, mat)) return 0;
	m.tri_uv.push_back(uv_a); m.tri_uv.push_back(uv_b); m.tri_uv.push_back(uv_c);     // uv_offsets_.push_back x3
	return 1;
}
yafaray_bool_t yafaray_startTriMeshPtr(yafaray_interface_t *yi, unsigned int *id, int vertices, int triangles, yafaray_bool_t has_orco, yafaray_bool_t has_uv, int type, int obj_pass_index)
{	// interface.cc:153-160: the scene picks the id
	if(!id) return fail(yi, "startTriMeshPtr: null id");
	*id = yafaray_getNextFreeId(yi);
	return yafaray_startTriMesh(yi, *id, vertices, triangles, has_orco, has_uv, type, obj_pass_index);
}
// Scene::startCurveMesh, scene.cc:133-152: an object of its own, a TriangleObject with UVs and without orco, type 0 (visible, no base mesh).
// `vertices` only sizes the reference's reservations.
yafaray_bool_t yafaray_startCurveMesh(yafaray_interface_t *yi, unsigned int id, int vertices, int)
{
	if(yi->state == 3) return fail(yi, "startCurveMesh: a curve mesh is already open (endCurveMesh closes it)");
	if(yi->state == 2) return fail(yi, "startCurveMesh: a mesh is open (endTriMesh closes it)");
	if(yi->state != 1) return fail(yi, "startCurveMesh: wrong state (call it between startGeometry and endGeometry)");
	note_srand(yi, ++g_object_index_auto);          // the TriangleObject is an ObjectGeometric, object_geom.cc:39-43
	{	// meshes_[id] is one slot: a curve started under a mesh's or an instance's id takes its place
		auto it = yi->meshes.find(id);
		if(it != yi->meshes.end()) { if(yi->last == &it->second) yi->last = nullptr; yi->meshes.erase(it); }
		yi->instances.erase(id);
	}
	Curve &c = yi->curves[id];
	c = Curve();
	c.points.reserve((size_t)std::max(vertices, 0) * 3);
	yi->cur_curve = &c; yi->cur_curve_id = id; yi->last_is_curve = true; yi->state = 3;
	yi->geometry_changed = true; yi->prepared = false; yi->scene_dirty = true;
	return 1;
}
// The two extrusion scales of point i of n, scene.cc:172-189.  Unqualified pow and sqrt there are the C double functions (<cmath> alone, no
// using-directive): the ratio and the exponent are floats widened to double, the sum is taken in double and narrowed to `float r`.
// h scales v and s scales u through operator*(float, Vec3): (float)(0.5 * r) and (float)(1.5 * r / sqrt(3.f)).
static void curve_scales(int i, int n, float strand_start, float strand_end, float strand_shape, float &h, float &s)
{
	float r;
	if(strand_shape < 0) r = (float)((double)strand_start + ::pow((double)((float)i / (float)(n - 1)), (double)(1 + strand_shape)) * (double)(strand_end - strand_start));
	else r = (float)((double)strand_start + (1 - ::pow((double)(((float)(n - i - 1)) / (float)(n - 1)), (double)(1 - strand_shape))) * (double)(strand_end - strand_start));
	h = (float)(0.5 * (double)r);
	s = (float)(1.5 * (double)r / ::sqrt((double)3.f));
}
// Scene::endCurveMesh, scene.cc:154-281.  The points, the material and the three floats are kept, with the scales above per point; the
// extrusion and the face fill run on the device when the scene is set up.  A refused call closes the block and drops the object.
yafaray_bool_t yafaray_endCurveMesh(yafaray_interface_t *yi, const yafaray_material_t *mat, float strand_start, float strand_end, float strand_shape)
{
	if(yi->state != 3) return fail(yi, "endCurveMesh: no curve mesh is open (startCurveMesh opens one)");
	Curve &c = *yi->cur_curve;
	const unsigned int id = yi->cur_curve_id;
	auto refuse = [&](const std::string &why) { yi->curves.erase(id); yi->cur_curve = nullptr; yi->last_is_curve = false; yi->state = 1; return fail(yi, "endCurveMesh: " + why); };
	const int n = (int)(c.points.size() / 3);
	if(!mat) return refuse("null material (the reference stores it in every triangle and dereferences it at the first hit)");
	if(n < 2) return refuse("a curve needs two or more points, this one has " + std::to_string(n) + " (scene.cc:174 divides by n - 1)");
	for(size_t k = 0; k < c.points.size(); ++k)
		if(!std::isfinite(c.points[k])) return refuse("non-finite coordinate in point " + std::to_string(k / 3));
	if(!std::isfinite(strand_start) || !std::isfinite(strand_end) || !std::isfinite(strand_shape)) return refuse("non-finite strand_start, strand_end or strand_shape");
	c.scales.resize((size_t)n * 2);
	for(int i = 0; i < n; ++i)
	{
		curve_scales(i, n, strand_start, strand_end, strand_shape, c.scales[2 * (size_t)i], c.scales[2 * (size_t)i + 1]);
		if(!std::isfinite(c.scales[2 * (size_t)i]) || !std::isfinite(c.scales[2 * (size_t)i + 1]))
			return refuse("strand_start, strand_end and strand_shape give a non-finite radius at point " + std::to_string(i));
	}
	c.mat = mat->index; c.strand_start = strand_start; c.strand_end = strand_end; c.strand_shape = strand_shape;
	yi->cur_curve = nullptr; yi->state = 1;
	return 1;
}
// extension: n_curves strands in one call, exactly the loop of getNextFreeId / startCurveMesh / addVertex per point / endCurveMesh
yafaray_bool_t yafaray_addCurves(yafaray_interface_t *yi, int n_curves, const int *n_points, const float *points, const yafaray_material_t *mat,
                                 float strand_start, float strand_end, float strand_shape, unsigned int *ids)
{
	if(n_curves < 0 || (n_curves > 0 && (!n_points || !points))) return fail(yi, "addCurves: bad argument");
	const float *p = points;
	for(int k = 0; k < n_curves; ++k)
	{
		if(n_points[k] < 0) return fail(yi, "addCurves: negative point count for curve " + std::to_string(k));
		const unsigned int id = yafaray_getNextFreeId(yi);
		if(ids) ids[k] = id;
		if(!yafaray_startCurveMesh(yi, id, n_points[k], 0)) return 0;
		for(int i = 0; i < n_points[k]; ++i, p += 3) yafaray_addVertex(yi, (double)p[0], (double)p[1], (double)p[2]);
		if(!yafaray_endCurveMesh(yi, mat, strand_start, strand_end, strand_shape)) return 0;
	}
	return 1;
}
// what endCurveMesh stored, for tests: per curve, in object-id order, a record of 32-bit words {id, point count n, material index,
// strand_start, strand_end, strand_shape (floats), then n times x y z h s (floats)}.  Whole records are written while they fit into
// max_words; *n_words (if given) is what all of them take.  Returns the number of curves.
int yafaray_getCurves(yafaray_interface_t *yi, void *out, int max_words, int *n_words)
{
	size_t at = 0;
	for(const auto &kv : yi->curves)
	{
		const Curve &c = kv.second;
		const size_t n = c.scales.size() / 2, len = 6 + 5 * n;      // an open curve has no scales yet: it shows with no points
		if(out && at + len <= (size_t)std::max(max_words, 0))
		{
			int32_t *w = (int32_t *)out + at;
			w[0] = (int32_t)kv.first; w[1] = (int32_t)n; w[2] = c.mat;
			const float f[3] = {c.strand_start, c.strand_end, c.strand_shape};
			std::memcpy(w + 3, f, sizeof f);
			for(size_t i = 0; i < n; ++i)
			{
				const float q[5] = {c.points[3 * i], c.points[3 * i + 1], c.points[3 * i + 2], c.scales[2 * i], c.scales[2 * i + 1]};
				std::memcpy(w + 6 + 5 * i, q, sizeof q);
			}
		}
		at += len;
	}
	if(n_words) *n_words = (int)at;
	return (int)yi->curves.size();
}
// Scene::addInstance, scene.cc:1105-1130.  No geometry-state check: the XML loader issues it at document level (import_xml.cc:450-460,
// :640-671).  Any mesh can be a base, flagged BASEMESH or not.
yafaray_bool_t yafaray_addInstance(yafaray_interface_t *yi, unsigned int base_object_id, const float *obj_to_world)
{
	if(yi->curves.count(base_object_id))
		return fail(yi, "addInstance: the base object " + std::to_string(base_object_id) + " is a curve mesh: its triangles exist only on the device, after the scene is set up, and there is no base mesh to take them from");
	if(yi->instances.count(base_object_id))
		return fail(yi, "addInstance: the base object " + std::to_string(base_object_id) + " is itself an instance; instances of instances are not built (TriangleObjectInstance takes a TriangleObject's own triangles, object_geom.cc:104-121)");
	auto base = yi->meshes.find(base_object_id);
	if(base == yi->meshes.end()) return fail(yi, "addInstance: base mesh for instance doesn't exist: " + std::to_string(base_object_id));
	if(!obj_to_world) return fail(yi, "addInstance: null matrix");
	for(int k = 0; k < 16; ++k)
		if(!std::isfinite(obj_to_world[k])) return fail(yi, "addInstance: non-finite matrix entry m" + std::to_string(k / 4) + std::to_string(k % 4));
	const unsigned int id = yafaray_getNextFreeId(yi);
	note_srand(yi, ++g_object_index_auto);          // TriangleObjectInstance is an ObjectGeometric: its constructor runs (object_geom.cc:39-43)
	Instance &in = yi->instances[id];
	in.base = base_object_id;
	std::memcpy(in.m, obj_to_world, sizeof in.m);
	// copied now (object_geom.cc:108-111): a base smoothed after this call leaves the instance unsmoothed
	const Mesh &b = base->second;
	in.has_orco = b.has_orco; in.has_uv = b.has_uv; in.smooth = b.smooth; in.normals_exported = b.normals_exported;
	yi->geometry_changed = true; yi->prepared = false; yi->scene_dirty = true;
	return 1;
}
// what addInstance stored, for tests: records of 22 words {own id, base id, has_orco, has_uv, is_smooth, normals_exported, 16 floats}
// in object-id order; returns the number of instances
int yafaray_getInstances(yafaray_interface_t *yi, void *out, int max_instances)
{
	const int n = (int)yi->instances.size();
	int i = 0;
	for(const auto &kv : yi->instances)
	{
		if(!out || i >= max_instances) break;
		const Instance &in = kv.second;
		int32_t w[22] = {(int32_t)kv.first, (int32_t)in.base, in.has_orco ? 1 : 0, in.has_uv ? 1 : 0, in.smooth ? 1 : 0, in.normals_exported ? 1 : 0};
		std::memcpy(&w[6], in.m, sizeof in.m);
		std::memcpy((char *)out + (size_t)i * sizeof w, w, sizeof w);
		++i;
	}
	return n;
}
unsigned int yafaray_createObject(yafaray_interface_t *yi, const char *) { fail(yi, "createObject: parametric objects (sphere) are outside the GPU path's scope (triangle meshes only)"); return 0u; }
void *yafaray_createVolumeRegion(yafaray_interface_t *yi, const char *) { fail(yi, "createVolumeRegion: volume regions are outside the GPU path's scope (volume integrator \"none\" only)"); return nullptr; }
// RenderEnvironment::createImageHandler (environment.cc) -> TgaHandler::factory (imagehandler_tga.cc:525-556), HdrHandler::factory,
// PngHandler::factory: the same parameters in all three
yafaray_image_handler_t *yafaray_createImageHandler(yafaray_interface_t *yi, const char *name, yafaray_bool_t add_to_table)
{
	const ParamMap &p = yi->params;
	std::string type;
	if(!name) { fail(yi, "createImageHandler: null name"); return nullptr; }
	if(!p.get("type", type)) { fail(yi, "createImageHandler: type of image handler not specified (tga, hdr, pic and png files are written)"); return nullptr; }
	auto ih = std::make_shared<yafaray_image_handler>();
	if(type == "tga") ih->type = yafaray_image_handler::Tga;
	else if(type == "hdr" || type == "pic") ih->type = yafaray_image_handler::Hdr;
	else if(type == "png") ih->type = yafaray_image_handler::Png;
	else if(type == "jpg" || type == "jpeg" || type == "tif" || type == "tiff" || type == "exr")
	{ fail(yi, "createImageHandler: image type \"" + type + "\" has no encoder in this build (tga, hdr, pic and png files are written; JPEG, TIFF and OpenEXR need libraries this build lacks)"); return nullptr; }
	else { fail(yi, "createImageHandler: unknown image type \"" + type + "\" (tga, hdr, pic and png files are written)"); return nullptr; }
	if(add_to_table && yi->image_handlers.count(name)) { fail(yi, std::string("createImageHandler: an image handler named \"") + name + "\" already exists"); return nullptr; }
	int width = 0, height = 0; bool with_alpha = false, for_output = true, grayscale = false, denoise = false;
	p.get("width", width); p.get("height", height); p.get("alpha_channel", with_alpha); p.get("for_output", for_output);
	p.get("denoiseEnabled", denoise); p.get("img_grayscale", grayscale);
	if(denoise) { fail(yi, "createImageHandler: denoiseEnabled needs OpenCV, which this build lacks"); return nullptr; }
	if(grayscale) { fail(yi, "createImageHandler: img_grayscale: grey image files are not written (the combined pass is a colour image)"); return nullptr; }
	ih->for_output = for_output;
	if(for_output)
	{
		if(width < 1 || height < 1) { fail(yi, "createImageHandler: width " + std::to_string(width) + " and height " + std::to_string(height) + " must both be at least 1"); return nullptr; }
		if((uint64_t)width * (uint64_t)height > (1ull << 26)) { fail(yi, "createImageHandler: " + std::to_string(width) + " x " + std::to_string(height) + " is more than the 2^26 pixels an image may have"); return nullptr; }
		if(ih->type == yafaray_image_handler::Tga && (width > 65535 || height > 65535)) { fail(yi, "createImageHandler: a TGA file holds at most 65535 pixels a side"); return nullptr; }
		ih->width = width; ih->height = height;
		ih->alpha = with_alpha && ih->type != yafaray_image_handler::Hdr;      // (HdrHandler::saveToFile: "Ignoring alpha channel")
		try { ih->packed.assign((size_t)width * (size_t)height * 4, (uint8_t)0); }
		catch(...) { fail(yi, "createImageHandler: out of memory"); return nullptr; }
	}
	if(add_to_table) yi->image_handlers[name] = ih; else yi->loose_image_handlers.push_back(ih);
	return ih.get();
}

// ---- ImageOutput (common/output_image.cc) ---------------------------------------------------------------------------------------
namespace {

// ImageOutput::flush:106-114 for the combined pass with one view: the handler's saveToFile under the name as given.  `driven`: the pixels
// came one by one and are packed here, as the device's output stage would have packed them
bool image_output_save(yafaray_image_output *io)
{
	yafaray_image_handler &ih = *io->ih;
	io->err.clear();
	try
	{
		if(ih.driven)
		{
			const size_t n = (size_t)ih.width * (size_t)ih.height;
			for(size_t i = 0; i < n; ++i)
			{
				if(ih.type == yafaray_image_handler::Hdr) yafimg::pack_rgbe(&ih.rgba[4 * i], &ih.packed[4 * i]);
				else yafimg::pack_rgba8(&ih.rgba[4 * i], ih.alpha, &ih.packed[4 * i]);
			}
		}
		switch(ih.type)
		{
			case yafaray_image_handler::Tga: return yafimg::write_tga(io->path, ih.width, ih.height, ih.alpha, ih.packed.data(), io->err);
			case yafaray_image_handler::Hdr: return yafimg::write_hdr(io->path, ih.width, ih.height, ih.packed.data(), io->err);
			default: return yafimg::write_png(io->path, ih.width, ih.height, ih.alpha, ih.packed.data(), io->err);
		}
	}
	catch(...) {}
	try { io->err = "image file '" + io->path + "': out of memory"; } catch(...) {}
	return false;
}
// ImageOutput::putPixel (:39-45): image_->putPixel(x + b_x_, y + b_y_, col); a pixel outside the image is dropped
yafaray_bool_t image_output_put_pixel(void *user, int, int x, int y, float r, float g, float b, float a)
{
	yafaray_image_output *io = (yafaray_image_output *)user;
	if(!io) return 0;
	yafaray_image_handler &ih = *io->ih;
	const int64_t px = (int64_t)x + io->bx, py = (int64_t)y + io->by;
	if(px < 0 || py < 0 || px >= ih.width || py >= ih.height) return 1;
	try { if(ih.rgba.empty()) ih.rgba.assign((size_t)ih.width * (size_t)ih.height * 4, 0.f); }
	catch(...) { return 0; }
	ih.driven = true;
	float *o = &ih.rgba[4 * ((size_t)py * (size_t)ih.width + (size_t)px)];
	o[0] = r; o[1] = g; o[2] = b; o[3] = a;
	return 1;
}
void image_output_flush(void *user, int num_view)
{
	yafaray_image_output *io = (yafaray_image_output *)user;
	if(io && num_view == 0) (void)image_output_save(io);
}
// the image output behind a callback table: the table is recognised by its putPixel pointer
yafaray_image_output *image_output_of(const yafaray_output_t *out)
{
	return (out && out->putPixel == image_output_put_pixel) ? (yafaray_image_output *)out->user : nullptr;
}
int color_space_code(const std::string &cs) { return cs == "sRGB" ? 0 : (cs == "XYZ" ? 1 : (cs == "Raw_Manual_Gamma" ? 3 : 2)); }      // to_output_space's cases: anything else stays linear

} // namespace

yafaray_image_output_t *yafaray_createImageOutput(yafaray_interface_t *yi, yafaray_image_handler_t *handler, const char *path, int border_x, int border_y)
{
	if(!yi) return nullptr;
	if(!handler || !path || !*path) { fail(yi, "createImageOutput: null handler or empty path"); return nullptr; }
	std::shared_ptr<yafaray_image_handler> ih;
	for(const auto &kv : yi->image_handlers) if(kv.second.get() == handler) ih = kv.second;
	for(const auto &h : yi->loose_image_handlers) if(h.get() == handler) ih = h;
	if(!ih) { fail(yi, "createImageOutput: the handler is not one of this interface's image handlers (clearAll releases them)"); return nullptr; }
	if(!ih->for_output) { fail(yi, "createImageOutput: the image handler was made with for_output = false: it has no image to fill"); return nullptr; }
	if(border_x < 0 || border_y < 0) { fail(yi, "createImageOutput: negative border (" + std::to_string(border_x) + ", " + std::to_string(border_y) + ")"); return nullptr; }
	yafaray_image_output *io = new(std::nothrow) yafaray_image_output();
	if(!io) { fail(yi, "createImageOutput: out of memory"); return nullptr; }
	try { io->ih = ih; io->path = path; }
	catch(...) { delete io; fail(yi, "createImageOutput: out of memory"); return nullptr; }
	io->bx = border_x; io->by = border_y;
	io->table.user = io; io->table.putPixel = image_output_put_pixel; io->table.flush = image_output_flush;
	return io;
}
void yafaray_destroyImageOutput(yafaray_image_output_t *image_output) { delete image_output; }
const char *yafaray_imageOutputLastError(const yafaray_image_output_t *image_output) { return image_output ? image_output->err.c_str() : "null image output"; }
const yafaray_output_t *yafaray_imageOutputCallbacks(yafaray_image_output_t *image_output) { return image_output ? &image_output->table : nullptr; }

yafaray_bool_t yafaray_addTriangles(yafaray_interface_t *yi, int n_verts, const float *verts, int n_tris, const int *indices, const yafaray_material_t *mat)
{
	if(in_curve(yi, "addTriangles")) return 0;
	if(yi->state != 2) return fail(yi, "addTriangles: wrong state");
	if(!mat || !verts || !indices || n_verts < 0 || n_tris < 0) return fail(yi, "addTriangles: bad argument");
	Mesh &m = *yi->cur;
	const int base = (int)(m.points.size() / 3);
	m.points.insert(m.points.end(), verts, verts + (size_t)n_verts * 3);
	for(int i = 0; i < n_tris * 3; ++i)
	{
		if(indices[i] < 0 || indices[i] >= n_verts) return fail(yi, "addTriangles: vertex index out of range");
		m.tri.push_back(base + indices[i]);
	}
	m.tri_mat.insert(m.tri_mat.end(), (size_t)n_tris, mat->index);
	return 1;
}
// Scene::smoothMesh, scene.cc:383-543.  Vertex normals per triangle corner; a corner left without one (all-zero
// triple) uses the geometric normal, as Triangle::getSurface does for a negative normal index (triangle.cc:38-40).
// Parity unpinned: scene.cc does not build outside the reference's own build system; restated, and checked against an
// independent restatement in tests/test_host_api.py.
namespace {
inline void sub3(const float *a, const float *b, float *o) { o[0] = a[0] - b[0]; o[1] = a[1] - b[1]; o[2] = a[2] - b[2]; }
inline float len3(const float *v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }   // Vec3::length, vector.h (fSqrt__ = sqrt)
inline float sin_from_vectors(const float *a, const float *b)   // Vec3::sinFromVectors, vector.h:263-270
{
	const float div = (len3(a) * len3(b)) * 0.99999f + 0.00001f;
	float c[3]; cross3(a, b, c);
	float arg = (len3(c) / div) * 0.99999f;
	if(arg > 1.f) arg = 1.f;
	return (float)std::asin((double)arg);
}
}
yafaray_bool_t yafaray_smoothMesh(yafaray_interface_t *yi, unsigned int id, double angle_d)
{
	if(yi->state != 1) return fail(yi, "smoothMesh: wrong state (call it between endTriMesh and endGeometry)");
	Mesh *mp = nullptr;
	if((id && yi->curves.count(id)) || (!id && yi->last_is_curve))
		return fail(yi, "smoothMesh: the object is a curve mesh: its triangles are made on the device from the strand's points, and there are no stored faces to smooth");
	if(id && yi->instances.count(id)) return fail(yi, "smoothMesh: object " + std::to_string(id) + " is an instance: a TriangleObjectInstance has no normals of its own to smooth (it reads its base's)");
	if(id) { auto it = yi->meshes.find(id); if(it == yi->meshes.end()) return fail(yi, "smoothMesh: no such mesh"); mp = &it->second; }
	else { mp = yi->last; if(!mp) return fail(yi, "smoothMesh: no current mesh"); }
	Mesh &m = *mp;
	const float angle = (float)angle_d;
	const size_t nv = m.points.size() / 3, nt = m.tri.size() / 3;
	yi->geometry_changed = true; yi->prepared = false; yi->scene_dirty = true;
	if(m.normals_exported && m.normals.size() == m.points.size()) { m.smooth = true; return 1; }      // :402-406
	m.smooth_normals.assign(nt * 9, 0.f);
	m.smooth_by_vertex = angle >= 180.f;
	// face normals: Triangle::recNormal, triangle.h:295-302
	std::vector<float> fn(nt * 3);
	for(size_t t = 0; t < nt; ++t)
	{
		const float *a = &m.points[3 * (size_t)m.tri[3 * t]], *b = &m.points[3 * (size_t)m.tri[3 * t + 1]], *c = &m.points[3 * (size_t)m.tri[3 * t + 2]];
		float e1[3], e2[3]; sub3(b, a, e1); sub3(c, a, e2);
		cross3(e1, e2, &fn[3 * t]);
		normalize3(&fn[3 * t]);
	}
	auto corner_alpha = [&](size_t t, int q, int v1, int v2) {
		const float *pq = &m.points[3 * (size_t)m.tri[3 * t + (size_t)q]], *p1 = &m.points[3 * (size_t)m.tri[3 * t + (size_t)v1]], *p2 = &m.points[3 * (size_t)m.tri[3 * t + (size_t)v2]];
		float e1[3], e2[3]; sub3(p1, pq, e1); sub3(p2, pq, e2);      // PREPARE_EDGES, :383-384
		return sin_from_vectors(e1, e2);
	};
	auto normal_normalize = [](float *v) {   // Normal::normalize, vector.h:272-283
		float len = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
		if(len != 0.f) { len = (float)(1.0 / (double)std::sqrt(len)); v[0] *= len; v[1] *= len; v[2] *= len; }
	};
	if(angle >= 180.f)
	{	// :420-448
		std::vector<float> vn(nv * 3, 0.f);
		for(size_t t = 0; t < nt; ++t)
		{
			const int order[3][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}};
			for(int k = 0; k < 3; ++k)
			{
				const float alpha = corner_alpha(t, order[k][0], order[k][1], order[k][2]);
				float *dst = &vn[3 * (size_t)m.tri[3 * t + (size_t)k]];
				for(int c = 0; c < 3; ++c) dst[c] += fn[3 * t + (size_t)c] * alpha;
			}
		}
		for(size_t v = 0; v < nv; ++v) normal_normalize(&vn[3 * v]);
		for(size_t t = 0; t < nt; ++t)
			for(int k = 0; k < 3; ++k)
				for(int c = 0; c < 3; ++c) m.smooth_normals[9 * t + 3 * (size_t)k + (size_t)c] = vn[3 * (size_t)m.tri[3 * t + (size_t)k] + (size_t)c];
	}
	else if(angle > 0.1f)
	{	// :450-538 angle dependent smoothing
		const float thresh = host_fsin_poly((float)((double)angle * 0.01745329251994329576922) + (float)1.57079632679489661923);   // fCos__(DEG_TO_RAD(angle))
		std::vector<std::vector<uint32_t>> vface(nv);
		std::vector<std::vector<float>> alphas(nv);
		for(size_t t = 0; t < nt; ++t)
		{
			const int order[3][3] = {{0, 1, 2}, {1, 0, 2}, {2, 0, 1}};
			for(int k = 0; k < 3; ++k)
			{
				const size_t v = (size_t)m.tri[3 * t + (size_t)k];
				alphas[v].push_back(corner_alpha(t, order[k][0], order[k][1], order[k][2]));
				vface[v].push_back((uint32_t)t);
			}
		}
		std::vector<float> vnormals;      // the distinct normals found so far at this vertex
		for(size_t i = 0; i < nv; ++i)
		{
			const std::vector<uint32_t> &tris = vface[i];
			vnormals.clear();
			for(size_t j = 0; j < tris.size(); ++j)
			{
				const uint32_t f = tris[j];
				bool smooth = false;
				float vnorm[3] = {fn[3 * f] * alphas[i][j], fn[3 * f + 1] * alphas[i][j], fn[3 * f + 2] * alphas[i][j]};
				for(size_t k = 0; k < tris.size(); ++k)
				{
					const uint32_t f2 = tris[k];
					if(f2 == f) continue;                                   // Triangle::operator== compares indices (triangle.h:76-79)
					const float *n2 = &fn[3 * f2];
					if((fn[3 * f] * n2[0] + fn[3 * f + 1] * n2[1] + fn[3 * f + 2] * n2[2]) > thresh)
					{
						smooth = true;
						for(int c = 0; c < 3; ++c) vnorm[c] += n2[c] * alphas[i][k];
					}
				}
				if(!smooth) continue;                                       // n_idx = -1: the corner keeps the geometric normal
				normalize3(vnorm);
				const float *use = nullptr;
				for(size_t l = 0; l + 2 < vnormals.size(); l += 3)
					if((double)(vnorm[0] * vnormals[l] + vnorm[1] * vnormals[l + 1] + vnorm[2] * vnormals[l + 2]) > 0.999) { use = &vnormals[l]; break; }
				float chosen[3];
				if(use) { chosen[0] = use[0]; chosen[1] = use[1]; chosen[2] = use[2]; }
				else { chosen[0] = vnorm[0]; chosen[1] = vnorm[1]; chosen[2] = vnorm[2]; vnormals.insert(vnormals.end(), vnorm, vnorm + 3); }
				// :526-528: the first corner of f that is vertex i
				int corner = -1;
				for(int c = 0; c < 3; ++c) if((size_t)m.tri[3 * (size_t)f + (size_t)c] == i) { corner = c; break; }
				if(corner < 0) return fail(yi, "smoothMesh: mesh smoothing error");
				for(int c = 0; c < 3; ++c) m.smooth_normals[9 * (size_t)f + 3 * (size_t)corner + (size_t)c] = chosen[c];
			}
		}
	}
	m.smooth = true;
	return 1;
}
int yafaray_getLights(yafaray_interface_t *yi, void *out, int max_lights)
{
	const int n = (int)yi->light_order.size();
	for(int i = 0; out && i < std::min(n, max_lights); ++i) std::memcpy((char *)out + (size_t)i * sizeof(yafgpu_light), &yi->light_order[(size_t)i]->l, sizeof(yafgpu_light));
	return n;
}
yafaray_bool_t yafaray_getCamera(yafaray_interface_t *yi, const char *name, void *out)
{
	auto it = name ? yi->cameras.find(name) : yi->cameras.end();
	if(it == yi->cameras.end()) return fail(yi, "getCamera: no such camera");
	if(out) std::memcpy(out, &it->second->c.cam, sizeof(yafgpu_camera));
	return 1;
}
yafaray_bool_t yafaray_getBackground(yafaray_interface_t *yi, const char *name, void *out)
{
	auto it = name ? yi->backgrounds.find(name) : yi->backgrounds.end();
	if(it == yi->backgrounds.end()) return fail(yi, "getBackground: no such background");
	if(out) std::memcpy(out, &it->second->b.rec, sizeof(yafgpu_background));
	return 1;
}
yafaray_bool_t yafaray_getSky(yafaray_interface_t *yi, const char *name, void *out)
{
	auto it = name ? yi->backgrounds.find(name) : yi->backgrounds.end();
	if(it == yi->backgrounds.end()) return fail(yi, "getSky: no such background");
	if(out) std::memcpy(out, &it->second->b.sky, sizeof(yafgpu_sky));
	return 1;
}
yafaray_bool_t yafaray_getIntegratorAO(yafaray_interface_t *yi, const char *name, int *do_ao, int *samples, float *distance, float *color3)
{
	auto it = name ? yi->integrators.find(name) : yi->integrators.end();
	if(it == yi->integrators.end()) return fail(yi, "getIntegratorAO: no such integrator");
	const IntegratorCfg &c = it->second->c;
	if(do_ao) *do_ao = c.do_ao ? 1 : 0;
	if(samples) *samples = c.ao_samples;
	if(distance) *distance = c.ao_distance;
	if(color3) for(int k = 0; k < 3; ++k) color3[k] = c.ao_color[k];
	return 1;
}
yafaray_bool_t yafaray_getMaskMaterial(yafaray_interface_t *yi, const char *name, void *out8)
{
	auto it = name ? yi->materials.find(name) : yi->materials.end();
	if(it == yi->materials.end() || it->second->m.type != YAFGPU_MAT_MASKED) return fail(yi, "getMaskMaterial: no such mask_mat");
	const yafaray_material &mm = *it->second;
	if(out8)
	{
		int32_t w[8] = {mm.mask_sub[0], mm.mask_sub[1], 0, mm.m.sh_diffuse, mm.m.n_nodes, mm.m.receive_shadows, mm.m.visibility, (int32_t)mm.m.bsdf_flags};
		std::memcpy(&w[2], &mm.m.transmit_filter, 4);
		std::memcpy(out8, w, sizeof w);
	}
	return 1;
}
// an ieslight's parsed file (test hook for the parser): type, counts, max_rad_ and the largest vertical angle in radians, then up to n_floats
// of its pool layout: the horizontal map, the vertical map, the table row-major by horizontal angle
yafaray_bool_t yafaray_getIesLight(yafaray_interface_t *yi, const char *name, int *type, int *n_hor, int *n_vert, float *max_rad, float *max_v_angle, float *out, int n_floats)
{
	auto it = name ? yi->lights.find(name) : yi->lights.end();
	if(it == yi->lights.end() || (it->second->l.type != YAFGPU_LIGHT_IES && it->second->l.type != YAFGPU_LIGHT_IES_SOFT)) return fail(yi, "getIesLight: no such ieslight");
	const yafies::Data &d = it->second->ies;
	if(type) *type = d.type;
	if(n_hor) *n_hor = d.n_hor;
	if(n_vert) *n_vert = d.n_vert;
	if(max_rad) *max_rad = d.max_rad;
	if(max_v_angle) *max_v_angle = d.max_v_angle;
	if(out && n_floats > 0)
	{
		std::vector<float> all(d.hor);
		all.insert(all.end(), d.vert.begin(), d.vert.end()); all.insert(all.end(), d.table.begin(), d.table.end());
		std::memcpy(out, all.data(), sizeof(float) * std::min((size_t)n_floats, all.size()));
	}
	return 1;
}
yafaray_bool_t yafaray_getBlendMaterial(yafaray_interface_t *yi, const char *name, void *out10)
{
	auto it = name ? yi->materials.find(name) : yi->materials.end();
	if(it == yi->materials.end() || it->second->m.type != YAFGPU_MAT_BLEND) return fail(yi, "getBlendMaterial: no such blend_mat");
	const yafaray_material &bm = *it->second;
	if(out10)
	{
		int32_t w[10] = {bm.mask_sub[0], bm.mask_sub[1], 0, bm.m.n_nodes > 0 ? 1 : 0, bm.m.sh_diffuse, bm.m.n_nodes, bm.m.receive_shadows, bm.m.visibility,
		                 (int32_t)bm.m.bsdf_flags, bm.m.additional_depth};
		std::memcpy(&w[2], &bm.m.transmit_filter, 4);
		std::memcpy(out10, w, sizeof w);
	}
	return 1;
}
int yafaray_getMaterialTable(yafaray_interface_t *yi, void *out, int max_materials)
{
	std::vector<yafgpu_material> mats; std::vector<yafgpu_node> nodes;
	flatten_materials(yi, mats, nodes);
	const int n = (int)mats.size();
	for(int i = 0; out && i < std::min(n, max_materials); ++i) std::memcpy((char *)out + (size_t)i * sizeof(yafgpu_material), &mats[(size_t)i], sizeof(yafgpu_material));
	return n;
}
yafaray_bool_t yafaray_getMeshCornerNormals(yafaray_interface_t *yi, unsigned int id, float *out, int n_floats)
{
	auto it = yi->meshes.find(id);
	if(it == yi->meshes.end()) return fail(yi, "getMeshCornerNormals: no such mesh");
	const Mesh &m = it->second;
	if(m.smooth_normals.empty() || (int)m.smooth_normals.size() != n_floats) return fail(yi, "getMeshCornerNormals: the mesh has no smoothed normals of that size");
	std::memcpy(out, m.smooth_normals.data(), m.smooth_normals.size() * sizeof(float));
	return 1;
}

void yafaray_paramsSetPoint(yafaray_interface_t *yi, const char *name, double x, double y, double z) { Param p; p.type = Param::Point; p.v[0] = (float)x; p.v[1] = (float)y; p.v[2] = (float)z; set_param(yi, name, p); }
void yafaray_paramsSetString(yafaray_interface_t *yi, const char *name, const char *s) { Param p; p.type = Param::String; p.s = s ? s : ""; set_param(yi, name, p); }
void yafaray_paramsSetBool(yafaray_interface_t *yi, const char *name, yafaray_bool_t b) { Param p; p.type = Param::Bool; p.b = b != 0; set_param(yi, name, p); }
void yafaray_paramsSetInt(yafaray_interface_t *yi, const char *name, int i) { Param p; p.type = Param::Int; p.i = i; set_param(yi, name, p); }
void yafaray_paramsSetFloat(yafaray_interface_t *yi, const char *name, double f) { Param p; p.type = Param::Float; p.f = f; set_param(yi, name, p); }
void yafaray_paramsSetColor(yafaray_interface_t *yi, const char *name, float r, float g, float b, float a)
{	// interface.cc:247-252: Rgba::linearRgbFromColorSpace(input_color_space_, input_gamma_) (color.h:366-386); alpha stays
	float c[3] = {r, g, b};
	if(yi->input_color_space == 0)
	{	// linearRgbFromSRgb, color.h:352-357
		for(float &v : c) v = (v <= 0.04045f) ? (v / 12.92f) : host_fpow(((v + 0.055f) / 1.055f), 2.4f);
	}
	else if(yi->input_color_space == 1)
	{	// XYZ (D65) -> linear RGB, color.h:337-342,375-381
		static const float m[3][3] = {{3.2406255f, -1.537208f, -0.4986286f}, {-0.9689307f, 1.8757561f, 0.0415175f}, {0.0557101f, -0.2040211f, 1.0569959f}};
		const float o[3] = {c[0], c[1], c[2]};
		for(int k = 0; k < 3; ++k) c[k] = m[k][0] * o[0] + m[k][1] * o[1] + m[k][2] * o[2];
	}
	else if(yi->input_color_space == 3 && yi->input_gamma != 1.f)
		for(float &v : c) v = host_fpow(v, yi->input_gamma);      // gammaAdjust, color.h:101
	Param p; p.type = Param::Color; p.v[0] = c[0]; p.v[1] = c[1]; p.v[2] = c[2]; p.v[3] = a; set_param(yi, name, p);
}
void yafaray_paramsSetColorArray(yafaray_interface_t *yi, const char *name, const float *rgb, yafaray_bool_t with_alpha)
{	// interface.cc:254-259
	if(rgb) yafaray_paramsSetColor(yi, name, rgb[0], rgb[1], rgb[2], with_alpha ? rgb[3] : 1.f);
}
void yafaray_paramsSetMatrix(yafaray_interface_t *yi, const char *name, const float *m16, yafaray_bool_t transpose)
{	// interface.cc:260-289 (paramsSetMatrix / paramsSetMemMatrix, float): 16 values, row major
	if(!m16) return;
	Param p; p.type = Param::Matrix;
	for(int i = 0; i < 4; ++i) for(int j = 0; j < 4; ++j) p.m[4 * i + j] = transpose ? m16[4 * j + i] : m16[4 * i + j];
	set_param(yi, name, p);
}
void yafaray_paramsSetMatrixD(yafaray_interface_t *yi, const char *name, const double *m16, yafaray_bool_t transpose)
{	// the double overloads, interface.cc:266-289
	if(!m16) return;
	float f[16];
	for(int k = 0; k < 16; ++k) f[k] = (float)m16[k];
	yafaray_paramsSetMatrix(yi, name, f, transpose);
}
void yafaray_setInputColorSpace(yafaray_interface_t *yi, const char *color_space_string, float gamma_val)
{	// interface.cc:292-301
	const std::string cs = color_space_string ? color_space_string : "";
	if(cs == "sRGB") yi->input_color_space = 0;
	else if(cs == "XYZ") yi->input_color_space = 1;
	else if(cs == "LinearRGB") yi->input_color_space = 2;
	else if(cs == "Raw_Manual_Gamma") yi->input_color_space = 3;
	else yi->input_color_space = 0;
	yi->input_gamma = gamma_val;
}
void yafaray_paramsClearAll(yafaray_interface_t *yi) { yi->params.dicc.clear(); yi->eparams.clear(); yi->cparams = &yi->params; }
void yafaray_paramsStartList(yafaray_interface_t *yi) { yi->eparams.emplace_back(); yi->cparams = &yi->eparams.back(); }
void yafaray_paramsPushList(yafaray_interface_t *yi) { yi->eparams.emplace_back(); yi->cparams = &yi->eparams.back(); }
void yafaray_paramsEndList(yafaray_interface_t *yi) { yi->cparams = &yi->params; }

yafaray_material_t *yafaray_createMaterial(yafaray_interface_t *yi, const char *name)
{
	std::string type;
	if(!name) { fail(yi, "createMaterial: null name"); return nullptr; }
	if(yi->materials.count(name)) { fail(yi, std::string("createMaterial: \"") + name + "\" already defined"); return nullptr; }
	if(!yi->params.get("type", type)) { fail(yi, "createMaterial: type of material not specified"); return nullptr; }
	auto m = std::make_unique<yafaray_material>();
	bool ok;
	if(type == "shinydiffusemat") ok = make_shinydiffuse(yi, yi->params, m->m, m->nodes);
	else if(type == "glossy") ok = make_glossy(yi, yi->params, m->m, m->nodes);
	else if(type == "light_mat") ok = make_lightmat(yi->params, m->m);
	else if(type == "glass") ok = make_glass(yi, yi->params, m->m, m->nodes);
	else if(type == "rough_glass") ok = make_rough_glass(yi, yi->params, m->m, m->nodes);
	else if(type == "coated_glossy") ok = make_coated_glossy(yi, yi->params, m->m, m->nodes);
	else if(type == "mirror") ok = make_mirror(yi->params, m->m);
	else if(type == "mask_mat") ok = make_mask(yi, yi->params, *m);
	else if(type == "blend_mat") ok = make_blend(yi, yi->params, *m);
	else { fail(yi, "createMaterial: material type \"" + type + "\" is outside the GPU path's scope (shinydiffusemat, glossy, coated_glossy, glass, rough_glass, mirror, light_mat, mask_mat, blend_mat)"); return nullptr; }
	if(!ok) return nullptr;
	if(type != "shinydiffusemat" && type != "glossy" && type != "coated_glossy" && type != "glass" && type != "mask_mat" && type != "blend_mat") clear_shader_slots(m->m);
	note_srand(yi, ++g_material_index_auto);        // Material::Material, material.cc:53-57
	m->index = (int)yi->material_order.size();
	yafaray_material *raw = m.get();
	yi->material_order.push_back(raw);
	yi->materials[name] = std::move(m);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}
// ImageTexture::factory's parameters other than the image itself (texture_image.cc:559-563, :657-716)
static bool texture_params(yafaray_interface *yi, const ParamMap &p, yafgpu_texture &t)
{
	std::string intp, clip;
	p.get("interpolate", intp);
	if(intp == "bicubic" || intp == "mipmap_trilinear" || intp == "mipmap_ewa")
		return fail(yi, "createTexture: interpolate \"" + intp + "\" is not supported by the GPU path (none and bilinear are)");
	bool normalmap = false; p.get("normalmap", normalmap);
	t.normalmap = normalmap ? 1 : 0;                 // :563, :705
	t.interpolate = intp == "none" ? 0 : 1;          // bilinear is the default (:575)
	bool rot90 = false, even = false, odd = true, mirror_x = false, mirror_y = false, clamp = false;
	int xrep = 1, yrep = 1; double minx = 0.0, miny = 0.0, maxx = 1.0, maxy = 1.0, cdist = 0.0;
	float intensity = 1.f, contrast = 1.f, saturation = 1.f, hue = 0.f, fr = 1.f, fg = 1.f, fb = 1.f;
	p.get("xrepeat", xrep); p.get("yrepeat", yrep);
	p.get("cropmin_x", minx); p.get("cropmin_y", miny); p.get("cropmax_x", maxx); p.get("cropmax_y", maxy);
	p.get("rot90", rot90); p.get("clipping", clip); p.get("even_tiles", even); p.get("odd_tiles", odd); p.get("checker_dist", cdist);
	p.get("mirror_x", mirror_x); p.get("mirror_y", mirror_y);
	p.get("adj_mult_factor_red", fr); p.get("adj_mult_factor_green", fg); p.get("adj_mult_factor_blue", fb);
	p.get("adj_intensity", intensity); p.get("adj_contrast", contrast); p.get("adj_saturation", saturation); p.get("adj_hue", hue); p.get("adj_clamp", clamp);
	t.xrepeat = xrep; t.yrepeat = yrep; t.rot90 = rot90; t.mirror_x = mirror_x; t.mirror_y = mirror_y;
	t.checker_even = even; t.checker_odd = odd; t.checker_dist = (float)cdist;
	// setCrop (:218-223): float members compared with double literals
	t.cropminx = (float)minx; t.cropmaxx = (float)maxx; t.cropminy = (float)miny; t.cropmaxy = (float)maxy;
	t.cropx = ((double)t.cropminx != 0.0) || ((double)t.cropmaxx != 1.0);
	t.cropy = ((double)t.cropminy != 0.0) || ((double)t.cropmaxy != 1.0);
	// string2Cliptype__ (:533-543): TexClipMode { Extend, Clip, ClipCube, Repeat, Checker }, anything unknown repeats
	t.clip = clip == "extend" ? 0 : clip == "clip" ? 1 : clip == "clipcube" ? 2 : clip == "checker" ? 4 : 3;
	// Texture::setAdjustments, texture.h:142-190
	t.adj_int = intensity; t.adj_con = contrast; t.adj_sat = saturation; t.adj_hue = hue / 60.f; t.adj_clamp = clamp;
	t.adj_r = fr; t.adj_g = fg; t.adj_b = fb;
	t.adj_set = (intensity != 1.f || contrast != 1.f || saturation != 1.f || hue != 0.f || clamp || fr != 1.f || fg != 1.f || fb != 1.f) ? 1 : 0;
	return true;
}
static int color_space_from(const std::string &cs)
{	// texture_image.cc:609-613
	if(cs == "sRGB") return yafimg::kSrgb;
	if(cs == "XYZ") return yafimg::kXyz;
	if(cs == "LinearRGB") return yafimg::kLinearRgb;
	if(cs == "Raw_Manual_Gamma") return yafimg::kRawManualGamma;
	return yafimg::kSrgb;
}
static yafaray_texture_t *register_texture(yafaray_interface *yi, const char *name, std::unique_ptr<yafaray_texture> t)
{
	t->index = (int)yi->texture_order.size();
	yafaray_texture *raw = t.get();
	yi->texture_order.push_back(raw);
	yi->textures[name] = std::move(t);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}

// Interface::createTexture (interface.h:84) -> RenderEnvironment::createTexture (environment.cc:203-224) -> ImageTexture::factory
// (texture_image.cc:545-720).  Only type "image" is on the GPU path; the procedural textures are refused.
yafaray_texture_t *yafaray_createTexture(yafaray_interface_t *yi, const char *name)
{
	const ParamMap &p = yi->params;
	std::string type, file, cs = "Raw_Manual_Gamma", opt = "optimized";
	if(!name) { fail(yi, "createTexture: null name"); return nullptr; }
	if(yi->textures.count(name)) { fail(yi, std::string("createTexture: \"") + name + "\" already defined"); return nullptr; }
	if(!p.get("type", type)) { fail(yi, "createTexture: type of texture not specified"); return nullptr; }
	if(type != "image") { fail(yi, "createTexture: texture type \"" + type + "\" is outside the GPU path's scope (image textures only)"); return nullptr; }
	auto t = std::make_unique<yafaray_texture>();
	std::memset(&t->t, 0, sizeof t->t);
	if(!texture_params(yi, p, t->t)) return nullptr;
	double gamma = 1.0; bool gray = false;
	p.get("color_space", cs); p.get("gamma", gamma); p.get("filename", file); p.get("texture_optimization", opt); p.get("img_grayscale", gray);
	if(file.empty()) { fail(yi, "createTexture: required argument filename not found for image texture"); return nullptr; }
	yafimg::Image img;
	img.color_space = color_space_from(cs); img.gamma = (float)gamma; img.grayscale = gray;
	img.optimization = opt == "optimized" ? yafimg::kOptOptimized : (opt == "compressed" ? yafimg::kOptCompressed : yafimg::kOptNone);   // :615-618
	std::string err, path = file;
	{	// the reference opens the name as given (relative to the working directory); the XML loader adds the scene file's directory
		FILE *f = std::fopen(path.c_str(), "rb");
		if(f) std::fclose(f);
		else if(!yi->base_dir.empty() && !file.empty() && file[0] != '/') path = yi->base_dir + "/" + file;
	}
	if(!yafimg::load(path, img, err)) { fail(yi, "createTexture: " + err); return nullptr; }
	t->t.width = img.width; t->t.height = img.height;
	t->t.color_space = img.color_space; t->t.gamma = (float)gamma;      // ImageTexture(ih, interpolation, gamma, color_space) with HDR's forced LinearRgb (:600-606, :631)
	t->texels = std::move(img.texels);
	return register_texture(yi, name, std::move(t));
}

// Not in the reference's Interface: an image texture over texels the caller already holds (what its ImageHandler::getPixel would
// return, row major, RGBA float), with the current ParamMap's ImageTexture parameters.  For embedders with in-memory images and
// for the parity tests, which feed the reference harness's own buffers.
yafaray_texture_t *yafaray_createTextureFromMemory(yafaray_interface_t *yi, const char *name, int width, int height, const float *rgba)
{
	const ParamMap &p = yi->params;
	if(!name || !rgba || width <= 0 || height <= 0) { fail(yi, "createTextureFromMemory: bad arguments"); return nullptr; }
	if(yi->textures.count(name)) { fail(yi, std::string("createTexture: \"") + name + "\" already defined"); return nullptr; }
	auto t = std::make_unique<yafaray_texture>();
	std::memset(&t->t, 0, sizeof t->t);
	if(!texture_params(yi, p, t->t)) return nullptr;
	std::string cs = "Raw_Manual_Gamma"; double gamma = 1.0;
	p.get("color_space", cs); p.get("gamma", gamma);
	t->t.width = width; t->t.height = height; t->t.color_space = color_space_from(cs); t->t.gamma = (float)gamma;
	t->texels.assign(rgba, rgba + (size_t)width * (size_t)height * 4);
	return register_texture(yi, name, std::move(t));
}

// the decoded image behind a texture (test hook for the file decoders): width / height, and up to n_floats of its RGBA texels
yafaray_bool_t yafaray_getTextureImage(yafaray_interface_t *yi, const char *name, int *width, int *height, float *rgba, int n_floats)
{
	auto it = name ? yi->textures.find(name) : yi->textures.end();
	if(it == yi->textures.end()) return fail(yi, "getTextureImage: no such texture");
	if(width) *width = it->second->t.width;
	if(height) *height = it->second->t.height;
	if(rgba && n_floats > 0) std::memcpy(rgba, it->second->texels.data(), sizeof(float) * std::min((size_t)n_floats, it->second->texels.size()));
	return 1;
}
yafaray_light_t *yafaray_createLight(yafaray_interface_t *yi, const char *name)
{
	std::string type;
	if(!name) { fail(yi, "createLight: null name"); return nullptr; }
	if(yi->lights.count(name)) { fail(yi, std::string("createLight: \"") + name + "\" already defined"); return nullptr; }
	if(!yi->params.get("type", type)) { fail(yi, "createLight: type of light not specified"); return nullptr; }
	auto l = std::make_unique<yafaray_light>();
	bool enabled, photon_only = false; int object = 0; std::string file; float aim[3];
	// light_area.cc:69, light_point.cc:40,60 (and light_directional.cc:62, light_sun.cc:55, light_sphere.cc:73): a photon-only light gives illumSample / illuminate nothing (and still counts among the lights the
	// one-light estimator picks from): a photon-mapping setting, not taken over
	if(yi->params.get("photon_only", photon_only) && photon_only) { fail(yi, "createLight: photon_only lights are outside the GPU path's scope (photon mapping)"); return nullptr; }
	if(type == "arealight") enabled = make_arealight(yi->params, l->l);
	else if(type == "pointlight") enabled = make_pointlight(yi->params, l->l);
	else if(type == "directionallight") enabled = make_directionallight(yi->params, l->l);
	else if(type == "sunlight") enabled = make_sunlight(yi->params, l->l);
	else if(type == "spherelight") enabled = make_spherelight(yi->params, l->l);
	else if(type == "meshlight" && yi->params.get("object", object)) enabled = make_meshlight(yi->params, l->l, l->object);
	else if(type == "bgPortalLight" && yi->params.get("object", object)) enabled = make_portallight(yi->params, l->l, l->object);
	else if(type == "ieslight" && yi->params.get("file", file)) { if(!make_ieslight(yi, yi->params, l->l, l->ies, enabled)) return nullptr; }
	else if(type == "spotlight" && yi->params.getPoint("from", aim) && yi->params.getPoint("to", aim)) { if(!make_spotlight(yi, yi->params, l->l, enabled)) return nullptr; }
	else
	{	// (a meshlight or a bgPortalLight without an object has no mesh at all: the reference's dereferences a null distribution at its first sample;
		// an ieslight without a file has nothing to parse, and the reference's factory returns no light either; a spotlight without its from
		// or its to is the one deviation: the reference would aim it from the origin down -z, here the call that names neither stays refused)
		fail(yi, "createLight: " + std::string(type == "ieslight" ? "no file given: " : type == "spotlight" ? "from and to are not both given: " : "") + "light type \"" + type + "\" is outside the GPU path's scope (arealight, pointlight, directionallight, sunlight, spherelight, meshlight or bgPortalLight with the object it lights from, ieslight with the file it reads, and spotlight with the from and to it aims along)");
		return nullptr;
	}
	yafaray_light *raw = l.get();
	if(enabled) yi->light_order.push_back(raw);   // Scene::addLight only sees enabled lights (environment.cc:230-233)
	yi->lights[name] = std::move(l);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}
yafaray_camera_t *yafaray_createCamera(yafaray_interface_t *yi, const char *name)
{
	std::string type;
	if(!name) { fail(yi, "createCamera: null name"); return nullptr; }
	if(!yi->params.get("type", type)) { fail(yi, "createCamera: type of camera not specified"); return nullptr; }
	if(type != "perspective" && type != "architect" && type != "angular" && type != "equirectangular")
	{	// Camera::factory, camera.cc:34-44, knows "orthographic" too: not built yet
		fail(yi, "createCamera: camera type \"" + type + "\" is outside the GPU path's scope (perspective, architect, angular, equirectangular)");
		return nullptr;
	}
	auto c = std::make_unique<yafaray_camera>();
	const bool made = type == "perspective" ? make_camera(yi, yi->params, c->c.cam) : type == "architect" ? make_architect_camera(yi, yi->params, c->c.cam)
	                : make_panoramic_camera(yi, yi->params, type == "angular", c->c.cam);
	if(!made) return nullptr;
	yafaray_camera *raw = c.get();
	yi->cameras[name] = std::move(c);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}
// The light a background with `ibl` brings along: ConstantBackground::factory / TextureBackground::factory build a "bglight" ParamMap
// (samples, with_caustic, with_diffuse, abs_intersect = false, cast_shadows) and hand the light to Scene::addLight on the spot
// (background_constant.cc:71-85, background_texture.cc:133-162).  light_enabled is not among those parameters: BackgroundLight::factory's
// default (true) stands.  with_caustic / with_diffuse steer photon emission only, which this path does not have.
static void add_background_light(yafaray_interface *yi, const char *fixed_name, int samples, bool cast_shadows, float clamp_intersect)
{
	auto l = std::make_unique<yafaray_light>();
	std::memset(&l->l, 0, sizeof l->l);
	l->l.type = YAFGPU_LIGHT_BACKGROUND; l->l.samples = samples; l->l.cast_shadows = cast_shadows ? 1 : 0;
	l->l.clamp_intersect = clamp_intersect; l->l.abs_intersect = 0;
	// the reference's fixed name collides when a second background of the kind asks for a light (createLight returns null and the factory
	// dereferences it); here every one gets a name of its own and prepareRender refuses the scene
	std::string name = fixed_name;
	for(int k = 2; yi->lights.count(name); ++k) name = std::string(fixed_name) + "#" + std::to_string(k);
	yi->light_order.push_back(l.get());
	yi->lights[name] = std::move(l);
}
yafaray_background_t *yafaray_createBackground(yafaray_interface_t *yi, const char *name)
{
	std::string type;
	const ParamMap &p = yi->params;
	if(!name) { fail(yi, "createBackground: null name"); return nullptr; }
	if(!p.get("type", type)) { fail(yi, "createBackground: type of background not specified"); return nullptr; }
	// The two skies are built only when the call names what they stand on — a sunsky its `from`, a gradientback both its horizon_color and
	// its zenith_color — which every exporter writes; the bare call of either type stays refused, the one deviation from the reference's
	// defaults.  darksky, and a sunsky that adds its own sun, need the measured spectral tables the project does not have.
	float sky_from[3] = {1.f, 1.f, 1.f}, sky_horizon[3] = {1.f, 1.f, 1.f}, sky_zenith[3] = {0.4f, 0.5f, 1.f};
	const bool sunsky = type == "sunsky" && p.getPoint("from", sky_from);
	const bool has_horizon = p.getColor("horizon_color", sky_horizon), has_zenith = p.getColor("zenith_color", sky_zenith);
	const bool gradient = type == "gradientback" && has_horizon && has_zenith;
	if(type != "constant" && type != "textureback" && !sunsky && !gradient)
	{
		fail(yi, "createBackground: " + std::string(type == "sunsky" ? "from is not given: " : type == "gradientback" ? "horizon_color and zenith_color are not both given: " : "") +
		         "background type \"" + type + "\" is outside the GPU path's scope (constant, textureback, sunsky with the from it takes the sun's direction from, and gradientback with its horizon_color and zenith_color" +
		         (type == "darksky" ? "; darksky computes its colours from measured spectral tables, which the GPU path does not have" : "") + ")");
		return nullptr;
	}
	if(sunsky)
	{
		bool add_sun = false;
		if(p.get("add_sun", add_sun) && add_sun)
		{
			fail(yi, "createBackground: sunsky with add_sun = true takes the sun's colour from measured spectral tables, which the GPU path does not have; leave add_sun off and create a sunlight of your own in the same direction");
			return nullptr;
		}
	}
	auto b = std::make_unique<yafaray_background>();
	std::memset(&b->b, 0, sizeof b->b);
	yafgpu_background &rec = b->b.rec;
	bool ibl = false, cast_shadows = true, caus = true, diff = true; int ibl_sam = 16; float power = 1.f;
	p.get("ibl", ibl); p.get("ibl_samples", ibl_sam); p.get("cast_shadows", cast_shadows); p.get("with_caustic", caus); p.get("with_diffuse", diff);
	p.get("power", power);
	(void)diff;
	if(type == "constant")
	{	// ConstantBackground::factory, background_constant.cc:51-88
		float col[3] = {0, 0, 0};
		p.getColor("color", col);
		for(int k = 0; k < 3; ++k) b->b.color[k] = rec.color[k] = power * col[k];
		rec.kind = YAFGPU_BACKGROUND_CONSTANT; rec.power = power; rec.texture = -1;
		rec.has_ibl = ibl ? 1 : 0;
		rec.shoots_caustic = 1;          // :69: the constructor gets `true` whatever with_caustic says
		if(ibl) add_background_light(yi, "constantBackground_bgLight", ibl_sam, cast_shadows, 0.f);
	}
	else if(gradient)
	{	// GradientBackground::factory, background_gradient.cc:61-103: the ground colours default to the sky's, `power` goes into all four
		// colours, and the constructor gets `true` for with_caustic whatever the parameter says (:84)
		yafgpu_sky &k = b->b.sky;
		float ground_horizon[3] = {sky_horizon[0], sky_horizon[1], sky_horizon[2]}, ground_zenith[3] = {sky_zenith[0], sky_zenith[1], sky_zenith[2]};
		p.getColor("horizon_ground_color", ground_horizon); p.getColor("zenith_ground_color", ground_zenith);
		for(int j = 0; j < 3; ++j)
		{
			k.horizon[j] = sky_horizon[j] * power; k.zenith[j] = sky_zenith[j] * power;
			k.horizon_ground[j] = ground_horizon[j] * power; k.zenith_ground[j] = ground_zenith[j] * power;
			if(!std::isfinite(k.horizon[j]) || !std::isfinite(k.zenith[j]) || !std::isfinite(k.horizon_ground[j]) || !std::isfinite(k.zenith_ground[j]))
			{ fail(yi, "createBackground: gradientback: a colour times power is not finite"); return nullptr; }
		}
		rec.kind = YAFGPU_BACKGROUND_GRADIENT; rec.power = power; rec.texture = -1;
		rec.has_ibl = ibl ? 1 : 0; rec.shoots_caustic = 1;
		if(ibl) add_background_light(yi, "GradientBackground_bgLight", ibl_sam, cast_shadows, 0.f);
	}
	else if(sunsky)
	{	// SunSkyBackground::factory, background_sunsky.cc:181-264, and the constructor, :37-76, in double as there.  The light is asked for
		// by background_light / light_samples, not ibl / ibl_samples; power is a double parameter narrowed at the constructor call
		yafgpu_sky &k = b->b.sky;
		float turb = 4.f, av = 1.f, bv = 1.f, cv = 1.f, dv = 1.f, ev = 1.f;
		double dpower = 1.0;
		bool bgl = false; int bgl_samples = 8;
		p.get("turbidity", turb); p.get("power", dpower);
		p.get("a_var", av); p.get("b_var", bv); p.get("c_var", cv); p.get("d_var", dv); p.get("e_var", ev);
		p.get("background_light", bgl); p.get("light_samples", bgl_samples);
		if(sky_from[0] == 0.f && sky_from[1] == 0.f && sky_from[2] == 0.f)
		{ fail(yi, "createBackground: sunsky: from, the direction to the sun, is the zero vector"); return nullptr; }
		k.power = (float)dpower; k.turbidity = turb;
		for(int j = 0; j < 3; ++j) k.from[j] = sky_from[j];
		float sun[3] = {sky_from[0], sky_from[1], sky_from[2]};
		ref_normalize(sun);
		// fAcos__ (util_math_optimizations.h:255-261): the double acos of a float, narrowed
		const float theta_f = (double)sun[2] <= -1.0 ? (float)3.14159265358979323846 : (double)sun[2] >= 1.0 ? 0.0f : (float)std::acos((double)sun[2]);
		const double theta_s = (double)theta_f, theta_2 = theta_s * theta_s, theta_3 = theta_2 * theta_s;
		const double t = (double)turb, t_2 = (double)(turb * turb);      // (t_2_ = turb * turb is a float product)
		k.theta_s = theta_s;
		k.phi_s = std::atan2((double)sun[1], (double)sun[0]);
		const double chi = (4.0 / 9.0 - t / 120.0) * (3.14159265358979323846 - 2.0 * theta_s);
		k.zenith_Y = (4.0453 * t - 4.9710) * std::tan(chi) - 0.2155 * t + 2.4192;
		k.zenith_Y *= 1000;
		k.zenith_x = (0.00165 * theta_3 - 0.00375 * theta_2 + 0.00209 * theta_s) * t_2 +
		             (-0.02903 * theta_3 + 0.06377 * theta_2 - 0.03202 * theta_s + 0.00394) * t +
		             (0.11693 * theta_3 - 0.21196 * theta_2 + 0.06052 * theta_s + 0.25886);
		k.zenith_y = (0.00275 * theta_3 - 0.00610 * theta_2 + 0.00317 * theta_s) * t_2 +
		             (-0.04214 * theta_3 + 0.08970 * theta_2 - 0.04153 * theta_s + 0.00516) * t +
		             (0.15346 * theta_3 - 0.26756 * theta_2 + 0.06670 * theta_s + 0.26688);
		const double var[5] = {(double)av, (double)bv, (double)cv, (double)dv, (double)ev};
		const double c_Y[5][2] = {{0.17872, -1.46303}, {-0.35540, 0.42749}, {-0.02266, 5.32505}, {0.12064, -2.57705}, {-0.06696, 0.37027}};
		const double c_x[5][2] = {{-0.01925, -0.25922}, {-0.06651, 0.00081}, {-0.00041, 0.21247}, {-0.06409, -0.89887}, {-0.00325, 0.04517}};
		const double c_y[5][2] = {{-0.01669, -0.26078}, {-0.09495, 0.00921}, {-0.00792, 0.21023}, {-0.04405, -1.65369}, {-0.01092, 0.05291}};
		for(int j = 0; j < 5; ++j)
		{
			k.perez_Y[j] = (c_Y[j][0] * t + c_Y[j][1]) * var[j];
			k.perez_x[j] = (c_x[j][0] * t + c_x[j][1]) * var[j];
			k.perez_y[j] = (c_y[j][0] * t + c_y[j][1]) * var[j];
		}
		bool finite = std::isfinite(k.power) && std::isfinite(turb) && std::isfinite(k.theta_s) && std::isfinite(k.phi_s) && std::isfinite(k.zenith_x) && std::isfinite(k.zenith_y) && std::isfinite(k.zenith_Y);
		for(int j = 0; j < 5; ++j) finite = finite && std::isfinite(k.perez_x[j]) && std::isfinite(k.perez_y[j]) && std::isfinite(k.perez_Y[j]);
		for(int j = 0; j < 3; ++j) finite = finite && std::isfinite(sky_from[j]);
		if(!finite) { fail(yi, "createBackground: sunsky: from, turbidity, power or one of a_var .. e_var is not finite, or leaves the sky model a value that is not"); return nullptr; }
		rec.kind = YAFGPU_BACKGROUND_SUNSKY; rec.power = k.power; rec.texture = -1;
		rec.has_ibl = bgl ? 1 : 0; rec.shoots_caustic = 1;      // :220: the constructor gets `true` whatever with_caustic says
		if(bgl) add_background_light(yi, "sunsky_bgLight", bgl_samples, cast_shadows, 0.f);
	}
	else
	{	// TextureBackground::factory, background_texture.cc:91-165
		std::string texname, mapping;
		float rot = 0.f, ibl_blur = 0.f, ibl_clamp_sampling = 0.f;
		if(!p.get("texture", texname)) { fail(yi, "createBackground: no texture given for texture background (parameter \"texture\")"); return nullptr; }
		auto t = yi->textures.find(texname);
		if(t == yi->textures.end()) { fail(yi, "createBackground: texture '" + texname + "' for textureback does not exist"); return nullptr; }
		p.get("smartibl_blur", ibl_blur); p.get("ibl_clamp_sampling", ibl_clamp_sampling); p.get("rotation", rot);
		if(ibl_blur > 0.f) { fail(yi, "createBackground: smartibl_blur > 0 needs mip maps, which the GPU path does not have (set smartibl_blur to 0)"); return nullptr; }
		rec.kind = YAFGPU_BACKGROUND_TEXTURE; rec.texture = t->second->index; rec.power = power;
		rec.projection = (p.get("mapping", mapping) && (mapping == "probe" || mapping == "angular")) ? 1 : 0;      // Angular, else Spherical
		// the constructor, :33-39: M_PI * rotation_ is a double product, narrowed where fSin__ / fCos__ take it
		rec.rotation = 2.0f * rot / 360.f;
		const float arg = (float)(3.14159265358979323846 * (double)rec.rotation);
		rec.sin_r = host_fsin_poly(arg);
		rec.cos_r = host_fsin_poly(arg + (float)1.57079632679489661923);
		rec.has_ibl = ibl ? 1 : 0; rec.shoots_caustic = caus ? 1 : 0;
		if(ibl) add_background_light(yi, "textureBackground_bgLight", ibl_sam, cast_shadows, ibl_clamp_sampling > 0.f ? ibl_clamp_sampling : 0.f);
	}
	yafaray_background *raw = b.get();
	yi->backgrounds[name] = std::move(b);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}
yafaray_integrator_t *yafaray_createIntegrator(yafaray_interface_t *yi, const char *name)
{
	std::string type;
	if(!name) { fail(yi, "createIntegrator: null name"); return nullptr; }
	if(!yi->params.get("type", type)) { fail(yi, "createIntegrator: type of integrator not specified"); return nullptr; }
	auto it = std::make_unique<yafaray_integrator>();
	IntegratorCfg &c = it->c;
	c.type = type;
	const ParamMap &p = yi->params;
	if(type == "pathtracing" || type == "directlighting")
	{
		bool transp_shad = false, do_ao = false, caustics = false;
		std::string c_method;
		p.get("raydepth", c.raydepth); p.get("shadowDepth", c.shadow_depth); p.get("transpShad", transp_shad); p.get("do_AO", do_ao);
		p.get("bg_transp", c.bg_transp); p.get("bg_transp_refract", c.bg_transp_refract);
		c.transp_shad = transp_shad;     // checked against the materials at render time (TriKdTree::intersectTs, row K3)
		{	// integrator_direct_light.cc:204-207,220-223 / integrator_path_tracer.cc:355-358,375-378
			double ao_dist = 1.0;
			p.get("AO_samples", c.ao_samples); p.get("AO_distance", ao_dist); p.getColor("AO_color", c.ao_color);
			c.do_ao = do_ao; c.ao_distance = (float)ao_dist;
			// sampleAmbientOcclusion divides by the sample count (integrator_montecarlo.cc:1087); the device path counts the samples of an
			// estimate in 12 bits.  (pathtracing never samples it, but a sample count no integrator could use is refused all the same.)
			if(do_ao && c.ao_samples < 1) { fail(yi, "createIntegrator: AO_samples must be at least 1 (the ambient occlusion estimate is divided by it)"); return nullptr; }
			if(do_ao && c.ao_samples > 4095) { fail(yi, "createIntegrator: AO_samples above 4095 are not supported by the GPU path (it counts the samples of an estimate in 12 bits)"); return nullptr; }
		}
		if(type == "pathtracing")
		{	// PathIntegrator::factory, integrator_path_tracer.cc:349-422
			p.get("path_samples", c.path_samples); p.get("bounces", c.bounces);
			p.get("russian_roulette_min_bounces", c.rr_min_bounces); p.get("no_recursive", c.no_recursive);
			if(p.get("caustic_type", c_method) && (c_method == "photon" || c_method == "both"))
			{ fail(yi, "createIntegrator: photon caustics are not supported by the GPU path (use caustic_type=path or none)"); return nullptr; }
			c.trace_caustics = c_method != "none";      // absent or any other word: the constructor's Path stays (:36), preprocess() sets trace_caustics_ (:85)
		}
		else
		{
			p.get("caustics", caustics);
			if(caustics) { fail(yi, "createIntegrator: photon caustics are not supported by the GPU path"); return nullptr; }
		}
	}
	else if(type != "none")
	{
		fail(yi, "createIntegrator: integrator type \"" + type + "\" is outside the GPU path's scope (pathtracing, directlighting, none)");
		return nullptr;
	}
	yafaray_integrator *raw = it.get();
	yi->integrators[name] = std::move(it);
	yi->prepared = false; yi->scene_dirty = true;
	return raw;
}

void yafaray_clearAll(yafaray_interface_t *yi)
{
	if(yi->gpu) { yafgpu_scene_destroy(yi->gpu); yi->gpu = nullptr; }
	yi->materials.clear(); yi->material_order.clear(); yi->textures.clear(); yi->texture_order.clear(); yi->lights.clear(); yi->light_order.clear();
	yi->image_handlers.clear(); yi->loose_image_handlers.clear();      // (an image output keeps its handler)
	yi->cameras.clear(); yi->backgrounds.clear(); yi->integrators.clear(); yi->meshes.clear(); yi->instances.clear(); yi->curves.clear(); yi->cur_curve = nullptr; yi->last_is_curve = false;
	yi->params.dicc.clear(); yi->eparams.clear(); yi->cparams = &yi->params;
	yi->state = -1; yi->prepared = false; yi->scene_dirty = true; yi->geometry_changed = true; yi->film.clear();
}

void yafaray_getRandState(yafaray_interface_t *yi, int *srand_seed, int *skip)
{
	if(yi->user_srand >= 0) { if(srand_seed) *srand_seed = yi->user_srand; if(skip) *skip = yi->user_skip; return; }
	if(srand_seed) *srand_seed = yi->have_srand ? (int)(yi->last_srand & 0x7fffffffu) : -1;
	if(skip) *skip = yi->have_srand ? colour_loop_draws(yi->last_srand) : 0;
}
void yafaray_setRandState(yafaray_interface_t *yi, int srand_seed, int skip)
{
	yi->user_srand = srand_seed < 0 ? -1 : srand_seed;
	yi->user_skip = (srand_seed < 0 || skip < 0) ? 0 : skip;
	yi->prepared = false;
}
void yafaray_setSerialReplay(yafaray_interface_t *yi, yafaray_bool_t on) { yi->serial_replay = on != 0; yi->prepared = false; }
void yafaray_setPlaneExchange(yafaray_interface_t *yi, yafaray_plane_exchange_t fn, void *user)
{
	yi->exchange = fn; yi->exchange_user = user;
	if(yi->gpu) yafgpu_scene_set_exchange(yi->gpu, fn, user);
}
void yafaray_setComm(yafaray_interface_t *yi, yafaray_comm_t *comm)
{
	if(comm) yafaray_setPlaneExchange(yi, yafaray_commExchange, comm);
	else yafaray_setPlaneExchange(yi, nullptr, nullptr);
}
void yafaray_setShard(yafaray_interface_t *yi, int shard_index, int shard_count) { yi->shard_index = shard_index; yi->shard_count = std::max(1, shard_count); }

// ---- yafaray_prepareRender: select, read, flatten, describe, adopt --------------------------------------------------------------
// RenderEnvironment::setupScene (environment.cc:679-813) + createImageFilm (:456-584) + Scene::update (scene.cc:784-894)
namespace {

struct Selection { const CameraCfg *cam = nullptr; const IntegratorCfg *inte = nullptr; const BackgroundCfg *bg = nullptr; std::string bg_name; };

bool select_render(yafaray_interface *yi, Selection &sel)
{
	const ParamMap &p = yi->params;
	std::string name;
	if(!p.get("camera_name", name)) return fail(yi, "Specify a Camera!!");
	auto cam = yi->cameras.find(name);
	if(cam == yi->cameras.end()) return fail(yi, "Specify an _existing_ Camera!!");
	if(!p.get("integrator_name", name)) return fail(yi, "Specify an Integrator!!");
	auto inte = yi->integrators.find(name);
	if(inte == yi->integrators.end()) return fail(yi, "Specify an _existing_ Integrator!!");
	if(inte->second->c.type == "none") return fail(yi, "Integrator is no surface integrator!");
	if(!p.get("volintegrator_name", name)) return fail(yi, "Specify a Volume Integrator!");
	auto vol = yi->integrators.find(name);
	if(vol == yi->integrators.end() || vol->second->c.type != "none") return fail(yi, "volume integrators other than type \"none\" are not supported by the GPU path");
	const BackgroundCfg *bg = nullptr;
	if(p.get("background_name", name))
	{
		auto b = yi->backgrounds.find(name);
		if(b == yi->backgrounds.end()) return fail(yi, "please specify an _existing_ Background!!");
		bg = &b->second->b;
	}
	// One image-based-lighting background per scene, and it is the one in use.  (The reference adds a background's light when the
	// background is created, selected or not, and two of one kind collide on the light's fixed name.)
	int n_bg_lights = 0;
	for(auto *l : yi->light_order) if(l->l.type == YAFGPU_LIGHT_BACKGROUND) ++n_bg_lights;
	if(n_bg_lights > 1) return fail(yi, "render: more than one background was created with ibl; the GPU path takes one image-based-lighting background per scene");
	if(n_bg_lights == 1 && !(bg && bg->rec.has_ibl))
		return fail(yi, "render: a background created with ibl is not the one background_name selects; its light would shine without it");
	if(bg && bg->rec.has_ibl && bg->rec.kind == YAFGPU_BACKGROUND_CONSTANT && !((bg->rec.color[0] + bg->rec.color[1] + bg->rec.color[2]) * 0.333333f > 0.f))
		return fail(yi, "render: a constant background with ibl needs a colour with energy; this one is black (its light's distribution would divide by zero)");
	sel.cam = &cam->second->c; sel.inte = &inte->second->c; sel.bg = bg;
	sel.bg_name = bg ? name : std::string();
	return true;
}

// What the parameters say about the render: read into a value of its own, which reaches the interface only when nothing refused it
struct RenderSetup
{
	yafgpu_aa_schedule aa{};
	yafgpu_render_params rp{};
	std::string color_space, color_space2 = "Raw_Manual_Gamma"; float gamma = 1.f, gamma2 = 1.f;
	std::vector<int32_t> tile_rand0;
};

bool read_render_setup(yafaray_interface *yi, const Selection &sel, RenderSetup &su)
{
	const ParamMap &p = yi->params;
	int aa_passes = 1, aa_samples = 1, tile_size = 32, width = 320, height = 240, xstart = 0, ystart = 0;
	int base_offset = 0, node = 0;
	float filt_sz = 1.5f, shadow_bias = (float)0.0005, min_raydist = (float)0.00005, clamp_samples = 0.f, clamp_indirect = 0.f;
	bool auto_bias = true, auto_dist = true, premult = false;
	std::string filter = "box";
	p.get("AA_passes", aa_passes); p.get("AA_minsamples", aa_samples); p.get("AA_pixelwidth", filt_sz);
	p.get("width", width); p.get("height", height); p.get("xstart", xstart); p.get("ystart", ystart);
	p.get("filter_type", filter); p.get("tile_size", tile_size); p.get("premult", premult);
	p.get("AA_clamp_samples", clamp_samples); p.get("AA_clamp_indirect", clamp_indirect);
	p.get("adv_auto_shadow_bias_enabled", auto_bias); p.get("adv_shadow_bias_value", shadow_bias);
	p.get("adv_auto_min_raydist_enabled", auto_dist); p.get("adv_min_raydist_value", min_raydist);
	p.get("adv_base_sampling_offset", base_offset); p.get("adv_computer_node", node);
	su.color_space = yi->color_space; su.gamma = yi->gamma;      // the first colour space stays what an earlier call read
	p.get("color_space", su.color_space); p.get("gamma", su.gamma);
	p.get("color_space2", su.color_space2); p.get("gamma2", su.gamma2);
	// Scene::setAntialiasing (scene.cc:761-778), defaults of RenderEnvironment::setupScene (environment.cc:682-695,747-762)
	{
		yafgpu_aa_schedule &aa = su.aa;
		int inc = aa_samples, var_edge = 10, var_pix = 0; double threshold = 0.05;
		float floor_pct = 0.f, smf = 1.f, lmf = 1.f, dark_factor = 0.f; bool color_noise = false; std::string dark = "none";
		p.get("AA_inc_samples", inc); p.get("AA_threshold", threshold); p.get("AA_resampled_floor", floor_pct);
		p.get("AA_sample_multiplier_factor", smf); p.get("AA_light_sample_multiplier_factor", lmf);
		p.get("AA_detect_color_noise", color_noise); p.get("AA_dark_detection_type", dark); p.get("AA_dark_threshold_factor", dark_factor);
		p.get("AA_variance_edge_size", var_edge); p.get("AA_variance_pixels", var_pix);
		aa.passes = aa_passes; aa.inc_samples = inc; aa.threshold = (float)threshold; aa.resampled_floor = floor_pct;
		aa.sample_multiplier_factor = smf; aa.light_sample_multiplier_factor = lmf; aa.detect_color_noise = color_noise ? 1 : 0;
		aa.dark_detection_type = dark == "linear" ? 1 : (dark == "curve" ? 2 : 0);
		aa.dark_threshold_factor = dark_factor; aa.variance_edge_size = var_edge; aa.variance_pixels = var_pix;
		if(aa_passes < 1) return fail(yi, "render: AA_passes must be at least 1");
		aa.rand_srand = -1; aa.rand_skip = 0;
		if(yi->have_srand) { aa.rand_srand = (int32_t)(yi->last_srand & 0x7fffffffu); aa.rand_skip = colour_loop_draws(yi->last_srand); }
		if(yi->user_srand >= 0) { aa.rand_srand = yi->user_srand; aa.rand_skip = yi->user_skip; }      // yafaray_setRandState
	}
	int filter_type = YAFGPU_FILTER_BOX;      // RenderEnvironment::createImageFilm, environment.cc:537-541: unknown names default to box
	if(filter == "mitchell") filter_type = YAFGPU_FILTER_MITCHELL;
	else if(filter == "gauss") filter_type = YAFGPU_FILTER_GAUSS;
	else if(filter == "lanczos") filter_type = YAFGPU_FILTER_LANCZOS;
	if(premult) return fail(yi, "render: premultiplied alpha is not supported by the GPU path");
	(void)clamp_indirect;   // only clamps caustic-photon estimates (integrator_path_tracer.cc:160-165), which this path does not have
	const IntegratorCfg &ic = *sel.inte;
	yafgpu_render_params &rp = su.rp;
	std::memset(&rp, 0, sizeof rp);
	rp.integrator = ic.type == "pathtracing" ? YAFGPU_INTEGRATOR_PATH : YAFGPU_INTEGRATOR_DIRECT;
	rp.path_samples = ic.path_samples; rp.bounces = ic.bounces; rp.rr_min_bounces = ic.rr_min_bounces;
	rp.no_recursive = ic.no_recursive; rp.bg_transp = ic.bg_transp; rp.bg_transp_refract = ic.bg_transp_refract;
	rp.trace_caustics = (ic.type == "pathtracing" && ic.trace_caustics) ? 1 : 0;
	// ambient occlusion: DirectLightIntegrator::integrate alone samples it (integrator_direct_light.cc:145)
	rp.do_ao = (ic.type == "directlighting" && ic.do_ao) ? 1 : 0;
	rp.ao_samples = ic.ao_samples; rp.ao_distance = ic.ao_distance;
	for(int k = 0; k < 3; ++k) rp.ao_color[k] = ic.ao_color[k];
	if(rp.do_ao && yi->light_order.size() > 254)
		return fail(yi, "render: do_AO with more than 254 lights is not supported by the GPU path (ambient occlusion takes a light's place in an 8-bit count)");
	rp.width = width; rp.height = height; rp.xstart = xstart; rp.ystart = ystart;
	rp.aa_minsamples = aa_samples; rp.aa_pixelwidth = filt_sz; rp.filter_type = filter_type; rp.tile_size = tile_size;
	rp.base_sampling_offset = (uint32_t)base_offset + (uint32_t)node * 100000u;   // imagefilm.h:124
	rp.shadow_bias_auto = auto_bias; rp.shadow_bias = shadow_bias; rp.min_raydist_auto = auto_dist; rp.min_raydist = min_raydist;
	rp.aa_light_sample_multiplier = 1.f;
	rp.aa_clamp_samples = clamp_samples;
	rp.raydepth = ic.raydepth;
	rp.transp_shad = ic.transp_shad ? 1 : 0; rp.shadow_depth = ic.shadow_depth;
	if(sel.bg) { rp.has_background = 1; for(int k = 0; k < 3; ++k) rp.background[k] = sel.bg->color[k]; }
	rp.shard_index = yi->shard_index; rp.shard_count = yi->shard_count;
	rp.serial_replay = yi->serial_replay ? 1 : 0;
	// the first pass's rand() per tile, for callers that run single passes themselves (yafaray_renderPassDevice)
	const int nt = ((width + tile_size - 1) / std::max(tile_size, 1)) * ((height + tile_size - 1) / std::max(tile_size, 1));
	su.tile_rand0.assign((size_t)std::max(nt, 0), 0);
	if(su.aa.rand_srand >= 0 && nt > 0)
	{
		std::vector<int32_t> v((size_t)su.aa.rand_skip + (size_t)nt);
		yafgpu_glibc_rand((uint32_t)su.aa.rand_srand, (int32_t)v.size(), v.data());
		std::copy(v.begin() + su.aa.rand_skip, v.end(), su.tile_rand0.begin());
	}
	return true;
}

// One set of rows: corner vertices, materials, vertex normals and texture coordinates per triangle corner.  The plain arrays are one,
// the base pools of the instances another, which marks the corners whose normal has index 0 as well.
struct RowPool
{
	std::vector<float> verts, vnormals, uv, orco; std::vector<int32_t> mat; std::vector<uint8_t> index0;
	void append(const Mesh &m, bool with_normals, bool with_texcoords, bool mark_index0)
	{
		const float kNoOrco = std::numeric_limits<float>::quiet_NaN();
		const size_t nt = m.tri_mat.size();
		for(size_t t = 0; t < nt; ++t)
		{
			uint8_t zero_marks = 0;
			for(int c = 0; c < 3; ++c)
			{
				const int vi = m.tri[3 * t + (size_t)c];
				verts.push_back(m.points[3 * (size_t)vi]); verts.push_back(m.points[3 * (size_t)vi + 1]); verts.push_back(m.points[3 * (size_t)vi + 2]);
				if(with_normals)
				{
					if(m.smooth && !m.smooth_normals.empty())
					{
						for(int q = 0; q < 3; ++q) vnormals.push_back(m.smooth_normals[9 * t + 3 * (size_t)c + (size_t)q]);
						// the angle-dependent loop appends its normals behind one slot per vertex (scene.cc:417-418, :519): none of them has index 0
						if(m.smooth_by_vertex && vi == 0) zero_marks |= (uint8_t)(1u << c);
					}
					else if(m.normals_exported && m.normals.size() >= 3 * ((size_t)vi + 1))
					{
						vnormals.push_back(m.normals[3 * (size_t)vi]); vnormals.push_back(m.normals[3 * (size_t)vi + 1]); vnormals.push_back(m.normals[3 * (size_t)vi + 2]);
						if(vi == 0) zero_marks |= (uint8_t)(1u << c);      // with exported normals the index is the vertex index
					}
					else { vnormals.push_back(0.f); vnormals.push_back(0.f); vnormals.push_back(0.f); }
				}
			}
			if(with_normals && mark_index0) index0.push_back(zero_marks);
			mat.push_back(m.tri_mat[t]);
			if(with_texcoords)
			{
				for(int c = 0; c < 3; ++c)
				{
					const size_t vi = (size_t)m.tri[3 * t + (size_t)c];
					if(m.has_uv && m.tri_uv.size() >= 3 * (t + 1))
					{ const size_t ui = (size_t)m.tri_uv[3 * t + (size_t)c]; uv.push_back(m.uv[2 * ui]); uv.push_back(m.uv[2 * ui + 1]); }
					else { uv.push_back(c == 0 ? kNoOrco : 0.f); uv.push_back(0.f); }            // has_uv_ false (NaN marker): sp.u_ = sp.v_ = 0, implicit dPdU / dPdV, triangle.cc:103-111
					if(m.has_orco && m.orco.size() >= 3 * (vi + 1))
					{ orco.push_back(m.orco[3 * vi]); orco.push_back(m.orco[3 * vi + 1]); orco.push_back(m.orco[3 * vi + 2]); }
					else { orco.push_back(c == 0 ? kNoOrco : 0.f); orco.push_back(0.f); orco.push_back(0.f); }   // has_orco_ false: orco = the hit point
				}
			}
		}
	}
};

// Everything the scene descriptor points into
struct FlatScene
{
	RowPool plain, base;                        // Scene::update's flattened meshes, and the base meshes of the instances
	std::vector<yafgpu_segment> segments;       // the flattened scene in object-id order (yafgpu_instancing)
	std::vector<float> curve_points;            // xyz and the two extrusion scales per point
	std::vector<yafgpu_material> mats; std::vector<yafgpu_node> nodes;
	std::vector<yafgpu_texture> textures; std::vector<float> texels;
	std::vector<yafgpu_light> lights;
	std::vector<float> light_verts;             // the light-geometry pool: the corners of every mesh light's and portal's triangles (yafgpu_scene_desc::light_verts)
	std::vector<float> ies_tables;              // the IES lights' maps and tables (yafgpu_scene_desc::ies_tables)
	std::vector<int32_t> light_tri_mat;         // per triangle of the pool its material, filled once a portal is there (yafgpu_scene_desc::light_tri_mat)
	bool any_normals = false, base_normals = false, any_nodes = false, with_textures = false, instanced = false;
};

// MeshLight::init (light_meshlight.cc:75-86): the light's mesh, by now part of the flattened scene.  plain_first / scene_first: the mesh's rows
// in the plain arrays and in the scene; the corners go to the light-geometry pool.  The areas are summed here as the device will sum them
// (initIs, :60-68: float areas, a double sum), to refuse a mesh that has none before anything is allocated and to show area_ in getLights.
bool resolve_mesh_light(yafaray_interface *yi, const FlatScene &f, const std::map<unsigned int, std::array<int32_t, 3>> &mesh_rows, const yafaray_light &light,
                        yafgpu_light &rec, std::vector<float> &pool)
{
	const std::string who = "render: meshlight object " + std::to_string(light.object);
	auto rows = mesh_rows.find(light.object);
	if(rows == mesh_rows.end())
	{
		if(yi->curves.count(light.object) || yi->instances.count(light.object))
			return fail(yi, who + " is a curve mesh or an instance: their triangles exist on the device only, a mesh light needs a plain mesh");
		if(yi->meshes.count(light.object)) return fail(yi, who + " is a mesh that is not rendered (invisible, or the base of instances): it has no rows for the light to be hit on");
		return fail(yi, who + " names no mesh");
	}
	const int32_t plain_first = rows->second[0], scene_first = rows->second[1], count = rows->second[2];
	if(count <= 0) return fail(yi, who + " is a mesh with no triangles");
	const float *v = f.plain.verts.data() + 9 * (size_t)plain_first;
	double total_area = 0.0;
	for(int32_t i = 0; i < count; ++i, v += 9)
	{
		const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
		float n[3]; cross3(e1, e2, n);
		total_area += (double)(float)(0.5 * (double)std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
	}
	if(!((float)total_area > 0.f && std::isfinite((float)total_area))) return fail(yi, who + " is a mesh whose total area is zero or not finite: nothing to sample by area");
	rec.mesh_first = scene_first; rec.mesh_count = count; rec.mesh_pool = (int32_t)(pool.size() / 9);
	rec.area = (float)total_area;      // area_, for getLights: the device computes its own, bit-equal one (the expressions are IEEE operations on both sides)
	pool.insert(pool.end(), f.plain.verts.begin() + 9 * (ptrdiff_t)plain_first, f.plain.verts.begin() + 9 * ((ptrdiff_t)plain_first + count));
	return true;
}

// BackgroundPortalLight::init (light_background_portal.cc:79-96): the light's mesh, from the interface's meshes and not from the flattened
// scene: init hides the mesh, so its triangles have no scene rows and live in the light-geometry pool alone, corners and materials.  Only a
// mesh that was created invisible has one meaning: Scene::update (scene.cc:788-874) builds the tree before it runs Light::init, so a visible
// portal mesh is in the tree for the first render, stops its own shadow rays, and is gone after the next geometry update.
// The areas are summed as the device will sum them (initIs, :63-71), to refuse early and to show area_ in getLights.
bool resolve_portal_light(yafaray_interface *yi, const Selection &sel, const yafaray_light &light, yafgpu_light &rec, std::vector<float> &pool, std::vector<int32_t> &pool_mat)
{
	const std::string who = "render: bgPortalLight object " + std::to_string(light.object);
	if(!sel.bg) return fail(yi, "render: a bgPortalLight needs a background to take its colour from, and the scene has none (the reference dereferences a null background at the first sample)");
	auto it = yi->meshes.find(light.object);
	if(it == yi->meshes.end())
	{
		if(yi->curves.count(light.object) || yi->instances.count(light.object))
			return fail(yi, who + " is a curve mesh or an instance: their triangles exist on the device only, a portal needs a plain mesh");
		return fail(yi, who + " names no mesh");
	}
	const Mesh &m = it->second;
	if(m.base) return fail(yi, who + " is the base of instances: a portal needs a plain mesh of its own");
	if(m.visible)
		return fail(yi, who + " is a visible mesh: the reference hides a portal's mesh only after the first tree is built, so it would block its own shadow rays in the first render and be gone from the next; create the mesh invisible (startTriMesh type bit 0x0100), as exporters do");
	const size_t count = m.tri_mat.size();
	if(count == 0) return fail(yi, who + " is a mesh with no triangles");
	if(pool.size() / 9 + count > (size_t)INT32_MAX) return fail(yi, who + ": the light-geometry pool outgrows 2^31 triangles");
	RowPool rows;
	rows.append(m, false, false, false);
	const float *v = rows.verts.data();
	double total_area = 0.0;
	for(size_t i = 0; i < count; ++i, v += 9)
	{
		const float e1[3] = {v[3] - v[0], v[4] - v[1], v[5] - v[2]}, e2[3] = {v[6] - v[0], v[7] - v[1], v[8] - v[2]};
		float n[3]; cross3(e1, e2, n);
		total_area += (double)(float)(0.5 * (double)std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]));
	}
	if(!((float)total_area > 0.f && std::isfinite((float)total_area))) return fail(yi, who + " is a mesh whose total area is zero or not finite: nothing to sample by area");
	rec.mesh_count = (int32_t)count; rec.mesh_pool = (int32_t)(pool.size() / 9);
	rec.area = (float)total_area;
	pool_mat.resize(pool.size() / 9, 0);      // (the mesh lights' entries before this one: read by nothing)
	pool.insert(pool.end(), rows.verts.begin(), rows.verts.end());
	pool_mat.insert(pool_mat.end(), rows.mat.begin(), rows.mat.end());
	return true;
}

// Scene::update: flatten visible non-base meshes in object-id order (scene.cc:797-817)
bool flatten_scene(yafaray_interface *yi, const Selection &sel, FlatScene &f)
{
	for(auto &kv : yi->meshes) if(kv.second.normals_exported || (kv.second.smooth && !kv.second.smooth_normals.empty())) f.any_normals = true;
	// texture coordinates, only when some material evaluates shader nodes: per triangle corner UVs and orcos (yafgpu_scene_desc)
	for(auto *m : yi->material_order) if(!m->nodes.empty()) f.any_nodes = true;
	// instances (Scene::addInstance, scene.cc:1105-1130): the flattened scene becomes a list of segments in object-id order, plain meshes as
	// rows of the plain arrays, instances as rows of the base pools under their matrix; the device makes the triangles (yafgpu_instancing)
	std::map<unsigned int, std::pair<int32_t, int32_t>> base_rows;      // base id -> its rows of the pools
	for(auto &kv : yi->instances) if(kv.second.smooth || kv.second.normals_exported) f.base_normals = true;
	// curves (Scene::endCurveMesh, scene.cc:154-281): a segment per strand over the pool of its points and their extrusion scales; the
	// device extrudes them and fills the prisms
	auto mesh_it = yi->meshes.begin(); auto inst_it = yi->instances.begin(); auto curve_it = yi->curves.begin();
	std::map<unsigned int, std::array<int32_t, 3>> mesh_rows;      // flattened mesh id -> its first row of the plain arrays, its first row of the scene, its rows
	int64_t scene_rows = 0;
	while(mesh_it != yi->meshes.end() || inst_it != yi->instances.end() || curve_it != yi->curves.end())
	{
		// the object with the smallest id goes next (an id names one object)
		const unsigned int none = ~0u;
		const unsigned int mesh_id = mesh_it != yi->meshes.end() ? mesh_it->first : none, inst_id = inst_it != yi->instances.end() ? inst_it->first : none;
		const unsigned int curve_id = curve_it != yi->curves.end() ? curve_it->first : none;
		if(curve_it != yi->curves.end() && curve_id <= mesh_id && curve_id <= inst_id)
		{
			const Curve &c = (curve_it++)->second;
			const size_t n = c.points.size() / 3;
			yafgpu_segment sg{}; sg.kind = YAFGPU_SEGMENT_CURVE; sg.first = (int32_t)(f.curve_points.size() / 5); sg.count = (int32_t)n; sg.flags = (uint32_t)c.mat;
			for(size_t i = 0; i < n; ++i)
			{
				f.curve_points.insert(f.curve_points.end(), c.points.begin() + 3 * (ptrdiff_t)i, c.points.begin() + 3 * (ptrdiff_t)i + 3);
				f.curve_points.push_back(c.scales[2 * i]); f.curve_points.push_back(c.scales[2 * i + 1]);
			}
			f.segments.push_back(sg);
			scene_rows += 6 * ((int64_t)n - 1) + 2;
			continue;
		}
		if(mesh_it != yi->meshes.end() && mesh_id <= inst_id)
		{
			const Mesh &m = mesh_it->second;
			const unsigned int id = (mesh_it++)->first;
			if(!m.visible || m.base) continue;
			yafgpu_segment sg{}; sg.kind = YAFGPU_SEGMENT_PLAIN; sg.first = (int32_t)f.plain.mat.size();
			f.plain.append(m, f.any_normals, f.any_nodes, false);
			sg.count = (int32_t)f.plain.mat.size() - sg.first;
			f.segments.push_back(sg);
			mesh_rows[id] = {sg.first, (int32_t)scene_rows, sg.count};
			scene_rows += sg.count;
			continue;
		}
		const Instance &in = (inst_it++)->second;      // visible_ is true whatever the base's visibility (object_geom.cc:112)
		auto base = yi->meshes.find(in.base);
		if(base == yi->meshes.end()) return fail(yi, "render: an instance's base mesh " + std::to_string(in.base) + " no longer exists");
		auto rows = base_rows.find(in.base);
		if(rows == base_rows.end())
		{
			const int32_t first = (int32_t)f.base.mat.size();
			f.base.append(base->second, f.base_normals, f.any_nodes, true);
			rows = base_rows.emplace(in.base, std::make_pair(first, (int32_t)f.base.mat.size() - first)).first;
		}
		yafgpu_segment sg{}; sg.kind = YAFGPU_SEGMENT_INSTANCE; sg.first = rows->second.first; sg.count = rows->second.second;
		sg.flags = ((in.smooth || in.normals_exported) ? (uint32_t)YAFGPU_INSTANCE_SMOOTH : 0u) | (in.has_orco ? (uint32_t)YAFGPU_INSTANCE_ORCO : 0u) | (in.has_uv ? (uint32_t)YAFGPU_INSTANCE_UV : 0u);
		std::memcpy(sg.m, in.m, sizeof sg.m);
		f.segments.push_back(sg);
		scene_rows += sg.count;
	}
	f.instanced = !yi->instances.empty() || !yi->curves.empty();
	if(yi->material_order.empty()) return fail(yi, "render: no materials defined");
	flatten_materials(yi, f.mats, f.nodes);
	f.with_textures = f.any_nodes || (sel.bg && sel.bg->rec.kind == YAFGPU_BACKGROUND_TEXTURE);
	if(f.with_textures)
		for(auto *t : yi->texture_order)
		{
			if((f.texels.size() + t->texels.size()) / 4 > 0xffffffffull) return fail(yi, "render: more than 2^32 texels in the scene's image textures");
			yafgpu_texture rec = t->t;
			rec.texel_first = (uint32_t)(f.texels.size() / 4);
			f.texels.insert(f.texels.end(), t->texels.begin(), t->texels.end());
			f.textures.push_back(rec);
		}
	for(auto *l : yi->light_order)
	{
		f.lights.push_back(l->l);
		if(l->l.type == YAFGPU_LIGHT_IES || l->l.type == YAFGPU_LIGHT_IES_SOFT)
		{	// the light's maps and table join the pool (the parser bounds one light's; 255 lights of the largest size stay below 2^31 floats)
			f.lights.back().ies_first = (int32_t)f.ies_tables.size();
			for(const std::vector<float> *v : {&l->ies.hor, &l->ies.vert, &l->ies.table}) f.ies_tables.insert(f.ies_tables.end(), v->begin(), v->end());
		}
		else if(l->l.type == YAFGPU_LIGHT_PORTAL)
		{
			if(!resolve_portal_light(yi, sel, *l, f.lights.back(), f.light_verts, f.light_tri_mat)) return false;
		}
		else if(l->l.type != YAFGPU_LIGHT_MESH) continue;
		else if(!resolve_mesh_light(yi, f, mesh_rows, *l, f.lights.back(), f.light_verts)) return false;
		l->l = f.lights.back();      // getLights shows the rows the light resolved to
	}
	if(!f.light_tri_mat.empty()) f.light_tri_mat.resize(f.light_verts.size() / 9, 0);
	return true;
}

yafgpu_scene_desc describe_scene(const FlatScene &f, const Selection &sel, int threads)
{
	yafgpu_scene_desc d{};
	d.n_tris = (int32_t)f.plain.mat.size(); d.verts = f.plain.verts.data(); d.tri_mat = f.plain.mat.data();
	d.vnormals = f.any_normals ? f.plain.vnormals.data() : nullptr;
	d.n_materials = (int32_t)f.mats.size(); d.materials = f.mats.data();
	d.n_lights = (int32_t)f.lights.size(); d.lights = f.lights.data();
	if(f.any_nodes)
	{
		d.tri_uv = f.plain.uv.data(); d.tri_orco = f.plain.orco.data();
		d.n_nodes = (int32_t)f.nodes.size(); d.nodes = f.nodes.data();
	}
	if(f.with_textures)
	{
		d.n_textures = (int32_t)f.textures.size(); d.textures = f.textures.data();
		d.n_texels = f.texels.size() / 4; d.texels = f.texels.data();
	}
	if(f.instanced)
	{
		d.inst.n_curve_points = (int32_t)(f.curve_points.size() / 5); d.inst.curve_points = f.curve_points.data();
		d.inst.n_segments = (int32_t)f.segments.size(); d.inst.segments = f.segments.data();
		d.inst.n_base_tris = (int32_t)f.base.mat.size(); d.inst.base_verts = f.base.verts.data(); d.inst.base_mat = f.base.mat.data();
		if(f.base_normals) { d.inst.base_vnormals = f.base.vnormals.data(); d.inst.base_vn_index0 = f.base.index0.data(); }
		if(f.any_nodes) { d.inst.base_uv = f.base.uv.data(); d.inst.base_orco = f.base.orco.data(); }
	}
	d.n_light_tris = (int32_t)(f.light_verts.size() / 9); d.light_verts = f.light_verts.data();
	d.light_tri_mat = f.light_tri_mat.empty() ? nullptr : f.light_tri_mat.data();
	d.n_ies_floats = (int32_t)f.ies_tables.size(); d.ies_tables = f.ies_tables.empty() ? nullptr : f.ies_tables.data();
	if(sel.bg) { d.background = sel.bg->rec; d.sky = sel.bg->sky; }
	d.camera = sel.cam->cam;
	d.build_threads = 0;
	if(threads > 0) d.build_threads = threads;
	return d;
}

} // namespace

// A call that fails leaves the interface unprepared, whatever an earlier call prepared.
yafaray_bool_t yafaray_prepareRender(yafaray_interface_t *yi)
{
	yi->prepared = false;
	Selection sel; RenderSetup su;
	if(!select_render(yi, sel) || !read_render_setup(yi, sel, su)) return 0;
	yi->aa = su.aa; yi->rp = su.rp; yi->tile_rand0 = std::move(su.tile_rand0);
	yi->color_space = su.color_space; yi->gamma = su.gamma; yi->color_space2 = su.color_space2; yi->gamma2 = su.gamma2;
	if(yi->state != 0) return fail(yi, "render: scene is not in the ready state (missing endGeometry?)");
	int threads = -1; yi->params.get("threads", threads);
	if(yi->gpu && !yi->scene_dirty && std::memcmp(&yi->scene_cam, &sel.cam->cam, sizeof yi->scene_cam) == 0 && yi->scene_threads == threads && yi->scene_background == sel.bg_name)
	{	// nothing the device scene is made of changed: keep it, tree and all (Scene::update rebuilds only on changes, scene.cc:784-790)
		yafgpu_scene_set_exchange(yi->gpu, yi->exchange, yi->exchange_user);
		yi->prepared = true;
		return 1;
	}
	if(yi->gpu) { yafgpu_scene_destroy(yi->gpu); yi->gpu = nullptr; }
	FlatScene flat;
	if(!flatten_scene(yi, sel, flat)) return 0;
	const yafgpu_scene_desc d = describe_scene(flat, sel, threads);
	if(yafgpu_scene_create(&d, &yi->gpu)) return fail(yi, std::string("scene upload: ") + yafgpu_last_error());
	yi->scene_dirty = false; yi->scene_cam = sel.cam->cam; yi->scene_threads = threads; yi->scene_background = sel.bg_name;
	yafgpu_scene_set_pass_pipelining(yi->gpu, yi->pass_pipelining);
	yafgpu_scene_set_abort_flag(yi->gpu, &yi->abort_flag);
	yafgpu_scene_set_exchange(yi->gpu, yi->exchange, yi->exchange_user);
	yafgpu_tree_info ti{};
	yafgpu_scene_info(yi->gpu, &ti);
	yi->stats = yafaray_render_stats_t{};
	yi->stats.tree_build_seconds = ti.build_seconds; yi->stats.upload_seconds = ti.upload_seconds;
	yi->stats.kd_nodes = ti.n_nodes; yi->stats.kd_leaf_refs = ti.n_leaf_refs; yi->stats.kd_max_depth = ti.max_depth; yi->stats.n_triangles = ti.n_tris;
	yi->stats.scene_device_bytes = ti.device_bytes;
	yi->prepared = true;
	return 1;
}

yafaray_bool_t yafaray_getRenderSize(yafaray_interface_t *yi, int *width, int *height)
{
	if(!yi->prepared) return fail(yi, "getRenderSize: call prepareRender first");
	if(width) *width = yi->rp.width;
	if(height) *height = yi->rp.height;
	return 1;
}

yafaray_bool_t yafaray_renderPassDevice(yafaray_interface_t *yi, float *d_planes, void *d_counters, void *stream)
{
	if(!yi->prepared) return fail(yi, "renderPassDevice: call prepareRender first");
	yi->rp.shard_index = yi->shard_index; yi->rp.shard_count = yi->shard_count;
	yi->rp.tile_rand = yi->tile_rand0.empty() ? nullptr : yi->tile_rand0.data();
	if(yafgpu_render_tiles(yi->gpu, &yi->rp, d_planes, (yafgpu_counters *)d_counters, stream)) return fail(yi, std::string("render: ") + yafgpu_last_error());
	return 1;
}

yafaray_bool_t yafaray_intersectRays(yafaray_interface_t *yi, int n, const float *rays, int *tri, float *t, float *bary)
{
	if(!yi->prepared) return fail(yi, "intersectRays: call prepareRender first");
	if(yafgpu_trace_closest(yi->gpu, n, rays, tri, t, bary)) return fail(yi, std::string("intersectRays: ") + yafgpu_last_error());
	return 1;
}
yafaray_bool_t yafaray_shadowRays(yafaray_interface_t *yi, int n, const float *rays, int *shadowed)
{
	if(!yi->prepared) return fail(yi, "shadowRays: call prepareRender first");
	if(yafgpu_trace_shadow(yi->gpu, n, rays, shadowed)) return fail(yi, std::string("shadowRays: ") + yafgpu_last_error());
	return 1;
}

yafaray_bool_t yafaray_setPassPipelining(yafaray_interface_t *yi, int mode)
{
	yi->pass_pipelining = mode < 0 ? -1 : (mode != 0 ? 1 : 0);
	if(yi->gpu) yafgpu_scene_set_pass_pipelining(yi->gpu, yi->pass_pipelining);
	return 1;
}
yafaray_bool_t yafaray_setProfiling(yafaray_interface_t *yi, yafaray_bool_t enable)
{
	if(!yi->prepared) return fail(yi, "setProfiling: call prepareRender first");
	return yafgpu_set_profiling(yi->gpu, enable) == 0;
}
yafaray_bool_t yafaray_getKernelProfile(yafaray_interface_t *yi, double ms[4], uint64_t launches[4])
{
	if(!yi->prepared) return fail(yi, "getKernelProfile: call prepareRender first");
	return yafgpu_get_profile(yi->gpu, ms, launches) == 0;
}

yafaray_bool_t yafaray_probe(yafaray_interface_t *yi, int op, int n, const float *in, int n_in, float *out, int n_out)
{
	if(!yi->prepared) return fail(yi, "probe: call prepareRender first");
	if(yafgpu_probe(yi->gpu, op, n, in, n_in, out, n_out)) return fail(yi, std::string("probe: ") + yafgpu_last_error());
	return 1;
}

// ImageFilm::flush (imagefilm.cc:737-772), combined pass: Pixel::normalized -> clampRgb0 -> Rgb::colorSpaceFromLinearRgb
// (color.h:388-411: sRGB via the polynomial fPow__, XYZ D65 by matrix, RawManualGamma by gammaAdjust(1 / gamma)) -> alpha
// clamped to [0, 1]
static void to_output_space(const std::string &cs, float gamma, float c[4])
{
	if(cs == "sRGB") { for(int k = 0; k < 3; ++k) c[k] = (c[k] <= 0.0031308f) ? (c[k] * 12.92f) : ((1.055f * host_fpow(c[k], 0.416667f)) - 0.055f); }
	else if(cs == "XYZ")
	{
		static const float m[3][3] = {{0.412400f, 0.357600f, 0.180500f}, {0.212600f, 0.715200f, 0.072200f}, {0.019300f, 0.119200f, 0.950500f}};
		const float o[3] = {c[0], c[1], c[2]};
		for(int k = 0; k < 3; ++k) c[k] = m[k][0] * o[0] + m[k][1] * o[1] + m[k][2] * o[2];
	}
	else if(cs == "Raw_Manual_Gamma" && gamma != 1.f)
	{
		if(gamma <= 0.f) gamma = 1.0e-2f;
		const float inv = 1.f / gamma;
		for(int k = 0; k < 3; ++k) c[k] = host_fpow(c[k], inv);
	}
	if(c[3] < 0.f) c[3] = 0.f; else if(c[3] > 1.f) c[3] = 1.f;
}
// why a render window at the output's border does not fit its handler's image ("" when it does): both sizes are named
static std::string image_output_misfit(const yafaray_image_output *io, int w, int h)
{
	const yafaray_image_handler &ih = *io->ih;
	if((int64_t)io->bx + w <= ih.width && (int64_t)io->by + h <= ih.height) return std::string();
	return "the render window of " + std::to_string(w) + " x " + std::to_string(h) + " at the border (" + std::to_string(io->bx) + ", " + std::to_string(io->by) +
	       ") does not fit the image handler's " + std::to_string(ih.width) + " x " + std::to_string(ih.height) + " (image file '" + io->path + "')";
}
// An upload of a host film, the output stage, a download: yafaray_filmToImage, and an image output whose scene holds the film no more
static bool film_to_image_uploaded(const float *film, const yafgpu_image_desc &desc, void *out, size_t out_bytes, std::string &err)
{
	if(!yafgpu_film_to_image) { err = "no device unit in this build (the output stage is a device kernel)"; return false; }
	const size_t film_bytes = (size_t)desc.width * (size_t)desc.height * 5 * sizeof(float);
	void *d_film = nullptr, *d_image = nullptr;
	hipError_t e = hipMalloc(&d_film, film_bytes);
	if(e == hipSuccess) e = hipMalloc(&d_image, out_bytes);
	if(e == hipSuccess) e = hipMemcpy(d_film, film, film_bytes, hipMemcpyHostToDevice);
	bool ok = e == hipSuccess;
	if(!ok) err = std::string("device memory for the film and the image: ") + hipGetErrorString(e);
	if(ok && yafgpu_film_to_image((const float *)d_film, &desc, d_image, nullptr)) { ok = false; err = yafgpu_last_error(); }
	if(ok && (e = hipMemcpy(out, d_image, out_bytes, hipMemcpyDeviceToHost)) != hipSuccess) { ok = false; err = std::string("image download: ") + hipGetErrorString(e); }
	if(d_film) (void)hipFree(d_film);
	if(d_image) (void)hipFree(d_image);
	return ok;
}
// An image output as the output of a render: one kernel launch on the film the scene's render targets hold, one download into the
// handler's buffer, one file (ImageFilm::flush + ImageOutput::flush for the combined pass)
static bool deliver_image(yafaray_interface_t *yi, yafaray_image_output *io, const std::string &cs, float gamma)
{
	yafaray_image_handler &ih = *io->ih;
	const std::string misfit = image_output_misfit(io, yi->rp.width, yi->rp.height);
	if(!misfit.empty()) return fail(yi, "image output: " + misfit);
	yafgpu_image_desc d{};
	d.width = yi->rp.width; d.height = yi->rp.height; d.color_space = color_space_code(cs); d.gamma = gamma; d.alpha = ih.alpha ? 1 : 0;
	d.format = ih.type == yafaray_image_handler::Hdr ? YAFGPU_IMAGE_RGBE : YAFGPU_IMAGE_RGBA8;
	d.image_width = ih.width; d.image_height = ih.height; d.border_x = io->bx; d.border_y = io->by;
	if(!yafgpu_scene_film_to_image) return fail(yi, "image output: no device unit in this build (the output stage is a device kernel)");
	const int rc = yi->gpu ? yafgpu_scene_film_to_image(yi->gpu, &d, ih.packed.data()) : -13;
	if(rc == -13)
	{	// the scene holds no film of this frame (-13): it was rebuilt or released since the render, so the host's copy of the film goes up again
		std::string why;
		if(!film_to_image_uploaded(yi->film.data(), d, ih.packed.data(), ih.packed.size(), why)) return fail(yi, "image output: " + why);
	}
	else if(rc) return fail(yi, std::string("image output: ") + yafgpu_last_error());
	ih.driven = false;
	if(!image_output_save(io)) return fail(yi, "image output: " + io->err);
	return true;
}
static bool deliver_to(yafaray_interface_t *yi, const yafaray_output_t *out, const std::string &cs, float gamma)
{
	if(!out) return true;
	if(yafaray_image_output *io = image_output_of(out)) return deliver_image(yi, io, cs, gamma);
	const int w = yi->rp.width, h = yi->rp.height;
	if(out->putPixel)
	{
		for(int y = 0; y < h; ++y)
			for(int x = 0; x < w; ++x)
			{
				const float *px = &yi->film[5 * ((size_t)y * (size_t)w + (size_t)x)];
				float c[4] = {0, 0, 0, 0};
				if(px[4] != 0.f) { const float f = (float)(1.0 / (double)px[4]); for(int k = 0; k < 4; ++k) c[k] = px[k] * f; }   // Pixel::normalized, Rgba / float (color.h:310-314)
				for(int k = 0; k < 3; ++k) c[k] = std::max(0.f, c[k]);              // clampRgb0
				to_output_space(cs, gamma, c);
				out->putPixel(out->user, 0, x, y, c[0], c[1], c[2], c[3]);
			}
	}
	if(out->flush) out->flush(out->user, 0);
	return true;
}
static bool deliver(yafaray_interface_t *yi, const yafaray_output_t *out)
{
	if(!deliver_to(yi, out, yi->color_space, yi->gamma)) return false;
	if(yi->has_output2) return deliver_to(yi, &yi->output2, yi->color_space2, yi->gamma2);      // Interface::setOutput2, interface.cc:420-423
	return true;
}

// ---- the rest of Interface's surface (interface.h:62-128): honoured where it touches this path, accepted where it only
// concerns logging / image decoration, refused with a diagnostic where it asks for something outside the scope
yafaray_bool_t yafaray_setLoggingAndBadgeSettings(yafaray_interface_t *yi)
{	// interface.cc:131-135 -> RenderEnvironment::setupLoggingAndBadge: log files and the parameters badge drawn onto saved
	// images — decoration of the output, not of the film; the settings are read and dropped
	std::string pos;
	if(yi->params.get("logging_paramsBadgePosition", pos)) yi->badge_position = pos;
	return 1;
}
yafaray_bool_t yafaray_setupRenderPasses(yafaray_interface_t *yi)
{	// interface.cc:137-141 -> RenderEnvironment::setupRenderPasses (environment.cc:598-677): with pass_enable the external
	// passes named by pass_* are rendered beside the combined one.  The GPU path produces the combined pass only.
	bool enable = false;
	yi->params.get("pass_enable", enable);
	if(!enable) return 1;
	for(const auto &kv : yi->params.dicc)
		if(kv.first.compare(0, 5, "pass_") == 0 && kv.second.type == Param::String && kv.second.s != "disabled" && kv.second.s != "combined")
			return fail(yi, "setupRenderPasses: render pass \"" + kv.first + "\" = \"" + kv.second.s + "\": the GPU path renders the combined pass only");
	return 1;
}
yafaray_bool_t yafaray_setInteractive(yafaray_interface_t *yi, yafaray_bool_t interactive) { yi->interactive = interactive != 0; return 1; }   // interface.cc:143-151
void yafaray_setConsoleVerbosityLevel(yafaray_interface_t *, const char *) {}      // interface.cc:374-377: console log level
void yafaray_setLogVerbosityLevel(yafaray_interface_t *, const char *) {}          // :379-382
void yafaray_setParamsBadgePosition(yafaray_interface_t *yi, const char *badge_position) { yi->badge_position = badge_position ? badge_position : "none"; }   // :384-387
yafaray_bool_t yafaray_getDrawParams(yafaray_interface_t *) { return 0; }           // :389-396: no badge is drawn
static void print_line(const char *level, const char *msg) { std::fprintf(stderr, "%s: %s\n", level, msg ? msg : ""); }
void yafaray_printDebug(yafaray_interface_t *, const char *msg) { if(std::getenv("YAFGPU_VERBOSE")) print_line("DEBUG", msg); }     // :425-449
void yafaray_printVerbose(yafaray_interface_t *, const char *msg) { if(std::getenv("YAFGPU_VERBOSE")) print_line("VERB", msg); }
void yafaray_printInfo(yafaray_interface_t *, const char *msg) { if(std::getenv("YAFGPU_VERBOSE")) print_line("INFO", msg); }
void yafaray_printParams(yafaray_interface_t *, const char *msg) { if(std::getenv("YAFGPU_VERBOSE")) print_line("PARM", msg); }
void yafaray_printWarning(yafaray_interface_t *, const char *msg) { print_line("WARNING", msg); }
void yafaray_printError(yafaray_interface_t *, const char *msg) { print_line("ERROR", msg); }
void yafaray_setOutput2(yafaray_interface_t *yi, const yafaray_output_t *out_2)
{	// interface.cc:420-423: a second ColorOutput, fed in colour space `color_space2` / `gamma2`
	yi->has_output2 = out_2 != nullptr;
	if(out_2) yi->output2 = *out_2;
}
int yafaray_getRenderParameters(yafaray_interface_t *yi, char *buf, int len)
{	// Interface::getRenderParameters (interface.h:111) hands out the ParamMap; across a C ABI: "name=value" lines.
	// Returns the number of bytes needed (excluding the terminator); writes at most len - 1 of them.
	std::string out;
	for(const auto &kv : yi->params.dicc)
	{
		out += kv.first + "=";
		const Param &q = kv.second;
		char tmp[160];
		switch(q.type)
		{
			case Param::Int: std::snprintf(tmp, sizeof tmp, "%d", q.i); out += tmp; break;
			case Param::Bool: out += q.b ? "true" : "false"; break;
			case Param::Float: std::snprintf(tmp, sizeof tmp, "%.9g", q.f); out += tmp; break;
			case Param::String: out += q.s; break;
			case Param::Point: std::snprintf(tmp, sizeof tmp, "%.9g %.9g %.9g", q.v[0], q.v[1], q.v[2]); out += tmp; break;
			case Param::Color: std::snprintf(tmp, sizeof tmp, "%.9g %.9g %.9g %.9g", q.v[0], q.v[1], q.v[2], q.v[3]); out += tmp; break;
			case Param::Matrix: for(int k = 0; k < 16; ++k) { std::snprintf(tmp, sizeof tmp, k ? " %.9g" : "%.9g", q.m[k]); out += tmp; } break;
			default: break;
		}
		out += "\n";
	}
	if(buf && len > 0) { const size_t n = std::min(out.size(), (size_t)len - 1); std::memcpy(buf, out.data(), n); buf[n] = 0; }
	return (int)out.size();
}

// ---- film files: ImageFilm::getFilmPath / imageFilmLoadAllInFolder / imageFilmFileBackup / imageFilmSave (imagefilm.cc:1330-1338,
// :1467-1557, :1659-1685, :1560-1657) around one yafaray_render.  The reader and the writer are yafimg::read_film / write_film.
static thread_local std::string g_film_err;      // yafaray_filmLastError: of this thread's last yafaray_readFilmFile / yafaray_writeFilmFile

static_assert(sizeof(yafaray_film_header_t) == sizeof(yafimg::FilmHeader), "yafaray_film_header_t is yafimg::FilmHeader");

static std::string film_file_of_node(const std::string &film_path, unsigned int node)
{
	char digits[16];
	std::snprintf(digits, sizeof digits, "%04u", node);      // setfill('0') << setw(4): wider numbers keep their digits
	return film_path + " - node " + digits + ".film";
}
// Path::Path(full_path) (file.cc:45-73): the directory up to the last separator, the base name up to the last dot, the extension
static void split_path(const std::string &full_path, std::string &dir, std::string &base, std::string &ext)
{
	std::string full_name = full_path;
	const size_t sep = full_path.find_last_of("\\/");
	dir.clear();
	if(sep != std::string::npos) { full_name = full_path.substr(sep + 1); dir = full_path.substr(0, sep); }
	if(dir.empty()) full_name = full_path;
	const size_t dot = full_name.find_last_of('.');
	if(dot != std::string::npos) { base = full_name.substr(0, dot); ext = full_name.substr(dot + 1); }
	else { base = full_name; ext.clear(); }
}
static bool is_regular_file(const std::string &path)
{
	struct stat st;
	return ::stat(path.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}

// the films a load-save render adds up, in the order they are added
struct FilmSource
{
	std::vector<std::string> files;      // accepted by their headers, sorted by path
	size_t next = 0;
	std::string warnings, error;
	// yafgpu_aa_schedule::resume_next: the next film's pass 0 into dst
	static int next_film(void *user, float *dst, uint64_t n_floats)
	{
		FilmSource *src = (FilmSource *)user;
		if(src->next >= src->files.size()) return 0;
		const std::string &path = src->files[src->next++];
		yafimg::FilmHeader hd;
		if(!yafimg::read_film(path, hd, dst, n_floats, src->error)) return -1;      // it passed the header check a moment ago
		return 1;
	}
};

// steps 1 and 2 of the loading, and the header checks: every regular file of the film path's directory with the extension "film" whose
// base name starts with the path's base name, sorted, less those whose header does not fit this render (a warning each)
static void collect_films(const std::string &film_path, const yafimg::FilmHeader &want, FilmSource &src, uint32_t &sampling_offset, uint32_t &base_sampling_offset)
{
	std::string dir, base, ext;
	split_path(film_path, dir, base, ext);
	if(dir.empty()) dir = ".";
	std::vector<std::string> found;
	if(DIR *d = ::opendir(dir.c_str()))
	{
		while(const dirent *e = ::readdir(d))
		{
			const std::string name = e->d_name, path = dir + "/" + name;
			std::string f_dir, f_base, f_ext;
			split_path(name, f_dir, f_base, f_ext);
			if(f_ext == "film" && f_base.rfind(base, 0) == 0 && is_regular_file(path)) found.push_back(path);
		}
		::closedir(d);
	}
	std::sort(found.begin(), found.end());
	for(const std::string &path : found)
	{
		yafimg::FilmHeader hd; std::string why;
		bool ok = yafimg::read_film(path, hd, nullptr, 0, why);
		if(ok && (hd.w != want.w || hd.h != want.h || hd.cx0 != want.cx0 || hd.cx1 != want.cx1 || hd.cy0 != want.cy0 || hd.cy1 != want.cy1))
		{
			ok = false;
			why = "film file '" + path + "' is of another frame: w " + std::to_string(hd.w) + " h " + std::to_string(hd.h) + " window x " + std::to_string(hd.cx0) + ".." +
			      std::to_string(hd.cx1) + " y " + std::to_string(hd.cy0) + ".." + std::to_string(hd.cy1) + ", the render has w " + std::to_string(want.w) + " h " +
			      std::to_string(want.h) + " window x " + std::to_string(want.cx0) + ".." + std::to_string(want.cx1) + " y " + std::to_string(want.cy0) + ".." + std::to_string(want.cy1);
		}
		if(!ok) { src.warnings += (src.warnings.empty() ? "film file skipped: " : "; film file skipped: ") + why; continue; }
		src.files.push_back(path);
		sampling_offset = std::max(sampling_offset, hd.sampling_offset);                   // imagefilm.cc:1546-1547
		base_sampling_offset = std::max(base_sampling_offset, hd.base_sampling_offset);
	}
}

// ImageFilm::sampling_offset_ after the render: offset + samples of the last renderPass that was called (integrator_tiled.cc:270); a pass
// that resamples no pixel is not called (:238) while acum advances all the same (:240)
static uint32_t stored_sampling_offset(const yafgpu_aa_schedule &aa, int aa_minsamples, bool resumed, uint32_t resume_offset, const std::vector<int32_t> &resampled)
{
	const int aa_samples = std::max(1, aa_minsamples), inc = aa.inc_samples > 0 ? aa.inc_samples : aa_samples;
	int acum = resumed ? (int)resume_offset : aa_samples;
	uint32_t stored = (uint32_t)acum;
	float sample_mult = 1.f;
	for(int i = 1; i < aa.passes; ++i)
	{
		sample_mult *= aa.sample_multiplier_factor;
		const int n = (int)std::ceil((float)inc * sample_mult);
		if((size_t)i < resampled.size() && resampled[(size_t)i] > 0) stored = (uint32_t)(acum + n);
		acum += n;
	}
	return stored;
}

static yafaray_bool_t render_checked(yafaray_interface_t *yi, const yafaray_output_t *output, const yafaray_progress_t *progress)
{
	// an abort that arrived before this call belongs to an earlier render (Scene::render clears the flag too, scene.cc:1040)
	yi->abort_flag = 0;
	yi->film_n_loaded = 0; yi->film_sampling_offset = 0u; yi->film_base_sampling_offset = 0u;
	// film files: without a film path the parameters have no effect (imagefilm.cc:900-904: an output that is no image file)
	std::string film_mode = "none", autosave = "none";
	yi->params.get("film_save_load", film_mode); yi->params.get("film_autosave_interval_type", autosave);
	const bool film_load = !yi->film_path.empty() && film_mode == "load-save";                      // environment.cc:524-526: any other word is "none"
	const bool film_save = !yi->film_path.empty() && (film_load || film_mode == "save");
	if(!yi->film_path.empty() && autosave != "none")
		return fail(yi, "render: film_autosave_interval_type = \"" + autosave + "\": saving the film between passes or on a timer is not supported by the GPU path (set it to \"none\")");
	if(film_save && yi->shard_count > 1)
		return fail(yi, "render: film_save_load = \"" + film_mode + "\" with a film path on a sharded frame (shard_count " + std::to_string(yi->shard_count) +
		                "): a rank's film is its share of the frame, not a film of the frame");
	// image outputs: what they cannot take is refused here, before anything is launched
	for(const yafaray_output_t *o : {output, yi->has_output2 ? (const yafaray_output_t *)&yi->output2 : nullptr})
		if(const yafaray_image_output *io = image_output_of(o))
		{
			std::string images_autosave = "none";
			yi->params.get("images_autosave_interval_type", images_autosave);
			if(images_autosave != "none")
				return fail(yi, "render: images_autosave_interval_type = \"" + images_autosave + "\": saving the image between passes or on a timer is not supported by the GPU path (set it to \"none\")");
			int width = 320, height = 240;      // read_render_setup's defaults
			yi->params.get("width", width); yi->params.get("height", height);
			const std::string misfit = image_output_misfit(io, width, height);
			if(!misfit.empty()) return fail(yi, "render: " + misfit);
		}
	if(progress && progress->init) progress->init(progress->user, 100);
	if(progress && progress->setTag) progress->setTag(progress->user, "Rendering...");
	if(!yafaray_prepareRender(yi)) return 0;
	if(yi->abort_flag) return fail(yi, "aborted");
	const int w = yi->rp.width, h = yi->rp.height;
	yi->film.assign((size_t)w * (size_t)h * 5, 0.f);
	int base_offset = 0, node = 0;
	yi->params.get("adv_base_sampling_offset", base_offset); yi->params.get("adv_computer_node", node);
	yafimg::FilmHeader hdr;
	hdr.computer_node = (uint32_t)node; hdr.base_sampling_offset = (uint32_t)base_offset; hdr.sampling_offset = 0u;
	hdr.w = w; hdr.h = h; hdr.cx0 = yi->rp.xstart; hdr.cx1 = yi->rp.xstart + w; hdr.cy0 = yi->rp.ystart; hdr.cy1 = yi->rp.ystart + h;
	FilmSource source;
	std::vector<float> first_film;
	yafgpu_aa_schedule aa = yi->aa;
	if(film_load)
	{
		collect_films(yi->film_path, hdr, source, hdr.sampling_offset, hdr.base_sampling_offset);
		if(!source.files.empty())
		{	// the first film goes straight to the device; the others follow through FilmSource::next_film, one at a time
			first_film.resize(yi->film.size());
			if(FilmSource::next_film(&source, first_film.data(), (uint64_t)first_film.size()) < 0) return fail(yi, "render: " + source.error);
			yi->film_n_loaded = (int)source.files.size();
			yi->film_sampling_offset = hdr.sampling_offset; yi->film_base_sampling_offset = hdr.base_sampling_offset;
			aa.resume_film = first_film.data(); aa.resume_sampling_offset = hdr.sampling_offset;
			if(source.next < source.files.size()) { aa.resume_next = FilmSource::next_film; aa.resume_user = &source; }
			yi->rp.base_sampling_offset = hdr.base_sampling_offset + (uint32_t)node * 100000u;      // imagefilm.h:124 over the merged value
		}
	}
	const std::string film_file = film_save ? film_file_of_node(yi->film_path, (unsigned int)node) : std::string();
	if(film_save && is_regular_file(film_file))
	{	// imageFilmFileBackup: the earlier film of this node stays at hand
		const std::string backup = film_file + "-previous.bak";
		auto name_of = [](const std::string &p) { const size_t sep = p.find_last_of("\\/"); return sep == std::string::npos ? p : p.substr(sep + 1); };
		if(std::rename(film_file.c_str(), backup.c_str()) != 0) source.warnings += std::string(source.warnings.empty() ? "" : "; ") + "film file backup to '" + backup + "' failed";
		else for(std::string &f : source.files) if(name_of(f) == name_of(film_file)) f += "-previous.bak";      // a film still to be added is read from where it is now
	}
	yafgpu_counters cn{};
	hipEvent_t e0, e1;
	(void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
	(void)hipEventRecord(e0, nullptr);
	yi->resampled.assign((size_t)std::max(1, yi->aa.passes), 0);
	const int rc = yafgpu_render_passes_to_host(yi->gpu, &yi->rp, &aa, yi->film.data(), &cn, yi->resampled.data());
	(void)hipEventRecord(e1, nullptr);
	(void)hipEventSynchronize(e1);
	float ms = 0.f; (void)hipEventElapsedTime(&ms, e0, e1);
	(void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
	if(rc) return fail(yi, std::string("render: ") + yafgpu_last_error() + (source.error.empty() ? "" : " (" + source.error + ")"));
	yi->stats.rays_closest = cn.rays_closest; yi->stats.rays_shadow = cn.rays_shadow; yi->stats.interior_steps = cn.interior_steps;
	yi->stats.leaves = cn.leaves; yi->stats.tri_tests = cn.tri_tests; yi->stats.camera_samples = cn.camera_samples; yi->stats.restarts = cn.restarts;
	yi->stats.render_seconds = (double)ms * 1e-3;
	if(film_save)
	{	// imageFilmSave, at the end of a render that finished
		hdr.sampling_offset = stored_sampling_offset(yi->aa, yi->rp.aa_minsamples, aa.resume_film != nullptr, aa.resume_sampling_offset, yi->resampled);
		std::string why;
		if(!yafimg::write_film(film_file, hdr, yi->film.data(), why)) return fail(yi, "render: " + why);
	}
	if(!source.warnings.empty()) yi->err = source.warnings;      // the render stands; the warnings are there to be read
	if(progress && progress->update) progress->update(progress->user, 100);
	if(progress && progress->done) progress->done(progress->user);
	if(!deliver(yi, output)) { yi->err = "render: " + yi->err; return 0; }      // an image file that could not be written fails the render
	return 1;
}

yafaray_bool_t yafaray_render(yafaray_interface_t *yi, const yafaray_output_t *output, const yafaray_progress_t *progress)
{
	try { return render_checked(yi, output, progress); }
	catch(const std::exception &e) { try { yi->err = std::string("render: ") + e.what(); } catch(...) {} }
	return 0;
}

void yafaray_setFilmPath(yafaray_interface_t *yi, const char *path) { yi->film_path = path ? path : ""; }
const char *yafaray_getFilmPath(const yafaray_interface_t *yi) { return yi->film_path.c_str(); }
void yafaray_getFilmResume(yafaray_interface_t *yi, int *n_loaded, unsigned int *sampling_offset, unsigned int *base_sampling_offset)
{
	if(n_loaded) *n_loaded = yi->film_n_loaded;
	if(sampling_offset) *sampling_offset = yi->film_sampling_offset;
	if(base_sampling_offset) *base_sampling_offset = yi->film_base_sampling_offset;
}
const char *yafaray_filmLastError(void) { return g_film_err.c_str(); }
yafaray_bool_t yafaray_writeFilmFile(const char *path, const yafaray_film_header_t *hdr, const float *film_hw5)
{
	try
	{
		g_film_err.clear();
		if(!path || !hdr) { g_film_err = "writeFilmFile: null argument"; return 0; }
		yafimg::FilmHeader hd;
		std::memcpy(&hd, hdr, sizeof hd);
		return yafimg::write_film(path, hd, film_hw5, g_film_err) ? 1 : 0;
	}
	catch(...) {}
	return 0;
}
yafaray_bool_t yafaray_readFilmFile(const char *path, yafaray_film_header_t *hdr, float *film_hw5, uint64_t n_floats)
{
	try
	{
		g_film_err.clear();
		if(!path || !hdr) { g_film_err = "readFilmFile: null argument"; return 0; }
		yafimg::FilmHeader hd;
		if(!yafimg::read_film(path, hd, film_hw5, n_floats, g_film_err)) return 0;
		std::memcpy(hdr, &hd, sizeof hd);
		return 1;
	}
	catch(...) {}
	return 0;
}

// a film the caller holds -> packed pixels, through the device's output stage (no interface, no scene)
yafaray_bool_t yafaray_filmToImage(const float *film_hw5, int w, int h, const char *color_space, float gamma, yafaray_bool_t alpha, int format, void *out)
{
	try
	{
		g_film_err.clear();
		if(!film_hw5 || !out || !color_space) { g_film_err = "filmToImage: null argument"; return 0; }
		if(w < 1 || h < 1 || (uint64_t)w * (uint64_t)h > (1ull << 26)) { g_film_err = "filmToImage: film size " + std::to_string(w) + " x " + std::to_string(h) + " out of range (1 x 1 to 2^26 pixels)"; return 0; }
		if(format != YAFGPU_IMAGE_FLOAT && format != YAFGPU_IMAGE_RGBA8 && format != YAFGPU_IMAGE_RGBE) { g_film_err = "filmToImage: unknown pixel format " + std::to_string(format); return 0; }
		const std::string cs = color_space;
		if(cs != "sRGB" && cs != "XYZ" && cs != "LinearRGB" && cs != "Raw_Manual_Gamma") { g_film_err = "filmToImage: unknown colour space \"" + cs + "\""; return 0; }
		yafgpu_image_desc d{};
		d.width = d.image_width = w; d.height = d.image_height = h; d.color_space = color_space_code(cs); d.gamma = gamma; d.alpha = alpha ? 1 : 0; d.format = format;
		const size_t out_bytes = (size_t)w * (size_t)h * (format == YAFGPU_IMAGE_FLOAT ? 16u : 4u);
		std::string why;
		if(film_to_image_uploaded(film_hw5, d, out, out_bytes, why)) return 1;
		g_film_err = "filmToImage: " + why;
	}
	catch(...) {}
	return 0;
}
// packed pixels -> an image file (host only)
yafaray_bool_t yafaray_writeImageFile(const char *path, const char *file_type, int w, int h, yafaray_bool_t alpha, const void *packed_pixels)
{
	try
	{
		g_film_err.clear();
		if(!path || !file_type) { g_film_err = "writeImageFile: null argument"; return 0; }
		const std::string type = file_type;
		bool ok = false;
		if(type == "tga") ok = yafimg::write_tga(path, w, h, alpha != 0, (const uint8_t *)packed_pixels, g_film_err);
		else if(type == "hdr" || type == "pic") ok = yafimg::write_hdr(path, w, h, (const uint8_t *)packed_pixels, g_film_err);
		else if(type == "png") ok = yafimg::write_png(path, w, h, alpha != 0, (const uint8_t *)packed_pixels, g_film_err);
		else g_film_err = "image type \"" + type + "\" has no encoder (tga, hdr, pic and png files are written)";
		if(!ok) g_film_err = "writeImageFile: " + g_film_err;
		return ok ? 1 : 0;
	}
	catch(...) {}
	return 0;
}

void yafaray_abort(yafaray_interface_t *yi) { yi->abort_flag = 1; }
void yafaray_internal_set_error(yafaray_interface_t *yi, const char *msg) { if(yi) yi->err = msg ? msg : ""; }
void yafaray_internal_set_base_dir(yafaray_interface_t *yi, const char *dir) { if(yi) yi->base_dir = dir ? dir : ""; }

yafaray_bool_t yafaray_getRenderedImage(yafaray_interface_t *yi, int num_view, const yafaray_output_t *output)
{
	if(num_view != 0 || yi->film.empty()) return fail(yi, "getRenderedImage: nothing rendered");
	if(!deliver(yi, output)) { yi->err = "getRenderedImage: " + yi->err; return 0; }
	return 1;
}
yafaray_bool_t yafaray_getFilm(yafaray_interface_t *yi, float *film, int width, int height)
{
	if(yi->film.empty() || width != yi->rp.width || height != yi->rp.height) return fail(yi, "getFilm: no film of that size");
	std::memcpy(film, yi->film.data(), yi->film.size() * sizeof(float));
	return 1;
}
yafaray_bool_t yafaray_getRenderStats(yafaray_interface_t *yi, yafaray_render_stats_t *stats)
{
	if(!stats) return 0;
	*stats = yi->stats;
	return 1;
}

} // extern "C"
