/* yafgpu.h — the narrow host<->device seam of the MI355X path-tracing core.
 *
 * This is the C ABI *inside* the drop-in ("second, narrower C ABI"): the wide,
 * Interface-shaped API in yafaray_c_api.h flattens a scene into the POD blocks below and calls
 * these entry points.  Plain pointers and sizes only; device buffers are raw HIP device pointers
 * so that a caller may own them (e.g. a torch tensor's data_ptr()) or let the library allocate.
 *
 * What each entry point replaces in the reference:
 *   yafgpu_scene_create   <- Scene::update()                (src/common/scene.cc:784-894): kd-tree
 *                            build (TriKdTree ctor, kdtree_triangle.cc:76-157) + Triangle cached
 *                            values (triangle.h:197-207) + Light::init
 *   yafgpu_render_tiles   <- TiledIntegrator::renderPass / renderTile
 *                            (src/integrator/integrator_tiled.cc:261-521) with
 *                            PathIntegrator::integrate (integrator_path_tracer.cc:112-347) and
 *                            ImageFilm::addSample (src/common/imagefilm.cc:925-1015) inside
 *   yafgpu_film_combine   <- the per-pixel sum that addSample performs across neighbouring samples
 *   yafgpu_trace_rays     <- Scene::intersect / Scene::isShadowed (scene.cc:896-994) on ray batches
 */
#ifndef YAFGPU_H
#define YAFGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YAFGPU_FILM_CHANNELS 5   /* r,g,b,a,weight : Pixel, include/utility/util_image_buffers.h:36-48 */
#define YAFGPU_FILM_PLANES   4   /* own, right, down, diagonal splat planes */

enum { YAFGPU_MAT_SHINYDIFFUSE = 0, YAFGPU_MAT_GLOSSY = 1, YAFGPU_MAT_LIGHT = 2, YAFGPU_MAT_GLASS = 3, YAFGPU_MAT_MIRROR = 4,
       YAFGPU_MAT_COATED_GLOSSY = 5, /* glossy's fields + mirror_color, mirror_strength, glass_ior = IOR, c_flags[0..2], n_bsdf */
       YAFGPU_MAT_ROUGH_GLASS = 6, /* glass's fields (glass_ior, filter_color, mirror_color, fake_shadow, beer_sigma) + rg_a2: RoughGlassMaterial, material_rough_glass.cc */
       /* MaskMaterial (material_mask.cc): a shader node's scalar picks one of two other records of the table at every hit.  Never a vertex's
          material: the device replaces it by the chosen record when it makes the vertex.  (Not "YAFGPU_MAT_MASK": that name is the shading
          units' compile-time set of material types, csrc/build.sh.)  The record adds no field; it reads
            c_index[0], c_index[1]   the records chosen for mask <= threshold / mask > threshold: hidden clones of material1 / material2 that
                                     carry the mask's material-level fields (see yafaray_c_api.cpp, flatten_materials)
            transmit_filter          threshold_, a float (material_mask.cc:30-31, :45)
            node_first, n_nodes      the nodes the mask shader reaches, in evaluation order;  sh_diffuse: the mask node's index among them
            is_transparent           isTransparent(): either sub-material's (:86-89)
            bsdf_flags               the union of both sub-materials' flags (:34)
            visibility, receive_shadows   the mask's own (:150-163); flat 0, additional_depth 0, no volume handler: its factory reads none */
       YAFGPU_MAT_MASKED = 7,
       /* BlendMaterial (material_blend.cc): every material function runs on two other records of the table and mixes the results by
          val (the constant blend_value, or a shader node's scalar at the hit) and ival = min(1, max(0, 1 - val)).  Unlike a mask it IS
          the vertex's material: the integrators read its material-level words, and the shading code reaches the two records through it
          (yafgpu_shading.h, BlendScratch).  Shading units handle it only when bit 8 of YAFGPU_MAT_MASK is set.  The record reads
            c_index[0], c_index[1]   hidden clones of material1 / material2 (yafaray_c_api.cpp, flatten_materials): the sub-materials as they
                                     are, nodes included, except flat, which becomes 2 (isFlat() is the blend's, false)
            transmit_filter          blend_val_, a float (material_blend.cc:45, :483)
            node_first, n_nodes      the nodes the `mask` shader reaches, in evaluation order; n_nodes 0: the constant blends
            sh_diffuse               the blend node's index among them (recalc_blend_, :518-526), -1 without one
            is_transparent           isTransparent(): either sub-material's (:332-335)
            bsdf_flags               the union of both sub-materials' flags (:42; initBsdf returns the same union, :100)
            additional_depth         the larger of the two (:48)
            has_vol_i, beer_sigma    getVolumeHandler(): material1's if both absorb and blend_val_ <= 0.5, else whichever exists (:450-462)
            visibility, receive_shadows   the blend's own (:485-499, :506); flat 0, no transparent bias: its factory reads neither */
       YAFGPU_MAT_BLEND = 8 };
enum { YAFGPU_LIGHT_AREA = 0, YAFGPU_LIGHT_POINT = 1, YAFGPU_LIGHT_DIRECTIONAL = 2, YAFGPU_LIGHT_SUN = 3, YAFGPU_LIGHT_SPHERE = 4,
       YAFGPU_LIGHT_BACKGROUND = 5, /* BackgroundLight (light_background.cc): samples the scene's yafgpu_background through its Pdf1D tables */
       /* MeshLight (light_meshlight.cc): a mesh of the scene sampled by area; its triangles and its Pdf1D row are in the light-geometry pool
          (yafgpu_scene_desc::light_verts).  Not 6: YAFGPU_LIGHT_BACKGROUND + 1 is the type that tests/scene_desc_cases.cpp hands
          yafgpu_scene_create as an unknown one, and it stays unknown */
       YAFGPU_LIGHT_MESH = 7,
       /* BackgroundPortalLight (light_background_portal.cc): a hidden mesh sampled by area that asks the scene's yafgpu_background for its
          colour.  Its triangles have no scene rows: corners, triangle records, normals and the Pdf1D row are all in the light-geometry pool */
       YAFGPU_LIGHT_PORTAL = 8,
       /* IesLight (light_ies.cc): a point with a measured distribution, a table looked up by two angles (yafgpu_scene_desc::ies_tables).
          Two types for its two behaviours, split by soft_shadows_: IES is a Dirac light (illuminate), IES_SOFT a sampled one that cannot be
          intersected (illumSample alone, the light half of the MIS pair, as the sphere light) */
       YAFGPU_LIGHT_IES = 9, YAFGPU_LIGHT_IES_SOFT = 10,
       /* SpotLight (light_spot.cc): a point light with a cone and a smoothstep falloff towards its edge.  Two types for its two behaviours,
          split by soft_shadows_ as the IES pair is: SPOT is a Dirac light (illuminate); SPOT_SOFT is sampled AND intersectable
          (canIntersect() == soft_shadows_, light_spot.h), so it takes both halves of the MIS pair, although its intersect() almost never
          answers true.  Not 13: the next unknown type stays unknown */
       YAFGPU_LIGHT_SPOT = 11, YAFGPU_LIGHT_SPOT_SOFT = 12 };
enum { YAFGPU_BACKGROUND_NONE = 0, YAFGPU_BACKGROUND_CONSTANT = 1, YAFGPU_BACKGROUND_TEXTURE = 2,
       /* The sky backgrounds: GradientBackground (background_gradient.cc) and SunSkyBackground (background_sunsky.cc, the Preetham model).
          Their constants are in yafgpu_scene_desc::sky, not in yafgpu_background.  Not 3: YAFGPU_BACKGROUND_TEXTURE + 1 is the kind that
          tests/scene_desc_cases.cpp hands yafgpu_scene_create as an unknown one, and it stays unknown */
       YAFGPU_BACKGROUND_GRADIENT = 4, YAFGPU_BACKGROUND_SUNSKY = 5 };
enum { YAFGPU_INTEGRATOR_PATH = 0, YAFGPU_INTEGRATOR_DIRECT = 1 };
enum { YAFGPU_FILTER_BOX = 0, YAFGPU_FILTER_MITCHELL = 1, YAFGPU_FILTER_GAUSS = 2, YAFGPU_FILTER_LANCZOS = 3 };

/* A material after its factory()/config() ran on the host (material_shiny_diffuse.cc:46-92,
 * material_glossy.cc:32-50, material_simple.cc:36-39).  64 floats, 16-byte aligned. */
typedef struct yafgpu_material
{
	int32_t type, visibility, receive_shadows, flat;      /* flat: 1 = flat_material; 2 = only the material's own test sees it (ShinyDiffuseMaterial::eval,
	                                                         material_shiny_diffuse.cc:275), not the integrator's isFlat(): a flat material under a mask */
	uint32_t bsdf_flags;
	int32_t n_bsdf;
	uint32_t c_flags[4];
	int32_t c_index[4];
	/* shinydiffuse */
	float diffuse_color[3], mirror_color[3], emit_color[3];
	float mirror_strength, transparency_strength, translucency_strength, diffuse_strength;
	float transmit_filter, ior_squared;
	int32_t is_mirror, is_transparent, is_translucent, is_diffuse, has_fresnel;
	int32_t use_oren;
	float oren_a, oren_b;
	/* glossy */
	float gloss_color[3], diff_color[3];
	float exponent, reflectivity, diffuse;
	int32_t as_diffuse, with_diffuse;
	int32_t anisotropic;           /* the Ashikhmin-Shirley lobe with exp_u / exp_v instead of Blinn (material_utils_microfacet.h:38-87) */
	float exp_u, exp_v;
	/* light material */
	float light_col[3];
	int32_t double_sided;
	/* glass (material_glass.cc:32-49; mirror_color = specular reflection colour) and mirror (mirror_color = colour * reflect) */
	float glass_ior;
	float filter_color[3];         /* transmit_filter * filter_color + (1 - transmit_filter) */
	int32_t fake_shadow;
	uint32_t tm_flags;             /* the transmission lobe: Filter|Transmit with fake shadows, else Specular|Transmit */
	int32_t has_vol_i;             /* glass "absorption": vol_i_ = BeerVolumeHandler (material_glass.cc:371-398), bsdf_flags has Volumetric */
	float beer_sigma[3];           /* its sigma_a_ = -log(absorption) / absorption_dist (volumehandler_beer.cc:28-35) */
	/* shader nodes: the material's nodes are nodes[node_first .. node_first + n_nodes) of the scene's node array,
	   in evaluation order (NodeMaterial::solveNodesOrder, material_node.cc:88-108); each shader slot names the node it reads
	   (index into that range) or -1.  shinydiffusemat slots, material_shiny_diffuse.cc:697-724. */
	int32_t node_first, n_nodes;
	int32_t sh_diffuse, sh_mirror_color, sh_mirror, sh_transparency, sh_translucency, sh_sigma_oren, sh_diffuse_refl, sh_ior;
	int32_t sh_glossy, sh_glossy_reflect, sh_exponent;      /* glossy / coated_glossy: glossy_shader, glossy_reflect_shader, exponent_shader (material_glossy.cc:504-511) */
	int32_t sh_filter_color;       /* glass: filter_color_shader (material_glass.cc:419-422) */
	int32_t bump_first, n_bump, sh_bump;   /* bump mapping: nodes[bump_first .. bump_first + n_bump) = what the bump shader reaches, in evaluation order
	                                          (NodeMaterial::evalBump, material_node.cc:132-139); sh_bump its index in that range; n_bump 0 = none */
	int32_t additional_depth;      /* Material::additional_depth_: recursiveRaytrace may go this much deeper below this material (integrator_montecarlo.cc:791) */
	float transp_bias_factor;      /* shinydiffusemat transparentbias_factor / transparentbias_multiply_raydepth (integrator_montecarlo.cc:1003-1011) */
	int32_t transp_bias_mult;
	float transp_ior;              /* glass: the index getTransparency's fresnel sees — ior_, or the IOR shader's value alone (material_glass.cc:223, sic) */
	float ior_base;                /* ior_ (the IOR shader adds to it, :258-262; coated_glossy: material_coated_glossy.cc:147) */
	float rg_a2;                   /* rough_glass: a_2_ = alpha^2 of its GGX lobe, alpha = max(1e-4, min(alpha / 2, 1)) (material_rough_glass.cc:33-36, :362) */
	float emit_strength;           /* emit_strength_ (emit() with a diffuse shader: colour * emit_strength_, :300) */
	int32_t has_diffuse_refl;      /* the fields below are only set in a resolved per-hit copy of the record (mat_resolve) */
	float diffuse_refl;
	int32_t oren_tex;              /* orenNayar with a texture's sigma: A and B in double (:230-235) */
	double oren_ad, oren_bd;
} yafgpu_material;

/* ImageTexture (src/texture/texture_image.cc) over float texels that hold what ImageHandler::getPixel returns (the host decoded
   the file, linearised its colours and pushed them through the image buffer's storage format) */
typedef struct yafgpu_texture
{
	int32_t width, height;
	uint32_t texel_first;          /* first texel in the scene's texel array (float4 units), row-major, row y = the handler's row y */
	int32_t interpolate;           /* 0 none, 1 bilinear */
	int32_t clip;                  /* TexClipMode: 0 extend, 1 clip, 2 clipcube, 3 repeat, 4 checker */
	int32_t xrepeat, yrepeat, rot90, mirror_x, mirror_y, checker_even, checker_odd;
	float checker_dist;
	int32_t cropx, cropy;
	float cropminx, cropmaxx, cropminy, cropmaxy;
	int32_t adj_set, adj_clamp;
	float adj_int, adj_con, adj_sat, adj_hue, adj_r, adj_g, adj_b;    /* adj_hue already divided by 60 (Texture::setAdjustments) */
	int32_t color_space;           /* for getRawColor / getFloat: 0 sRGB, 1 XYZ, 2 LinearRGB, 3 RawManualGamma */
	float gamma;
	int32_t normalmap;             /* texture_image.cc:705: a normal map (TextureMapperNode::evalDerivative reads the normal from its raw colour) */
} yafgpu_texture;

enum { YAFGPU_NODE_TEXTURE_MAPPER = 0, YAFGPU_NODE_VALUE = 1, YAFGPU_NODE_MIX = 2, YAFGPU_NODE_LAYER = 3 };
/* one shader node after its factory() / configInputs() ran on the host (shader_node_basic.cc, shader_node_layer.cc); node
   references are indices into the material's node range, -1 = not connected */
typedef struct yafgpu_node
{
	int32_t type;
	/* texture_mapper */
	int32_t texture, texco, mapping, map_x, map_y, map_z, do_scalar;
	float scale[3], offset[3];     /* offset already doubled (TextureMapperNode::factory :411) */
	float mtx[16];
	/* value */
	float color[4]; float value;
	/* mix */
	int32_t mode; float cfactor; int32_t input1, input2, factor;
	float col1[4], col2[4];
	/* layer */
	int32_t input, upper; uint32_t texflag;
	float colfac, valfac, def_val, upper_val;
	float def_col[4], upper_col[4];
	int32_t do_color, do_scalar_l, color_input, use_alpha;
	/* bump mapping (texture_mapper): what TextureMapperNode::setup leaves (shader_node_basic.cc:34-59): the texel steps 1 / width, 1 / height and
	   bump_strength / |scale| / 100 */
	float d_u, d_v, bump_str;
} yafgpu_node;

/* A light after its constructor ran on the host (light_area.cc:34-52, light_point.cc:28-36, light_directional.cc:31-42,
 * light_sun.cc:29-42, light_sphere.cc:31-41).  136 bytes whatever the type: the area light's corner block is overlaid by the
 * fields of the directional, sun and sphere lights.  Which fields each type reads:
 *   area         samples, corner, c2, c3, c4, to_x, to_y, fnormal, color (col * power * pi), area
 *   point        position (from), color (col * power)
 *   directional  direction (normalised), position (from) and radius when infinite == 0, color (col * power); du / dv are filled as the
 *                ctor does (createCs__ of the direction, light_directional.cc:39) and read by nothing here (photon emission only)
 *   sun          samples, direction (normalised), du / dv (createCs__ of the direction AS GIVEN, sic light_sun.cc:36), cos_angle,
 *                invpdf, pdf, col_pdf (color * pdf); color (col * power) is kept for reference only
 *   sphere       samples, position (center), radius, square_radius, square_radius_epsilon, color (col * power)
 *   background   samples, clamp_intersect (0 = no clamp), abs_intersect; what it emits is the scene's yafgpu_background
 *   mesh         samples, mesh_first, mesh_count, mesh_pool, double_sided, color (col * (float)power * pi); yafgpu_scene_create computes
 *                mesh_row and area (MeshLight::initIs, light_meshlight.cc:55-73) for the scene's own copy, whatever the caller wrote there
 *   portal       samples, mesh_count, mesh_pool, portal_power; yafgpu_scene_create computes mesh_first (here: where the light's triangle
 *                records start in the pool), mesh_row and area (BackgroundPortalLight::initIs, light_background_portal.cc:58-77).  No
 *                color: what it emits is the scene's yafgpu_background times portal_power; single-sided, so double_sided stays 0
 *   ies, ies_soft  samples (1 for ies), position (from), direction (ndir_ = normalize(from - to)), du / dv (createCs__ of dir_ = -ndir_),
 *                cos_angle (cos_end_ = fCos__ of the largest vertical angle), color (col * power), ies_first, ies_n_hor, ies_n_vert,
 *                ies_type, ies_max_rad
 *   spot, spot_soft  samples (1 for spot), position (from), direction (ndir_ = normalize(from - to)), du / dv (createCs__ of dir_ = -ndir_),
 *                cos_angle (cos_end_ = fCos__ of the cone angle), spot_cos_start (cos_start_, where the falloff begins), spot_icos_diff
 *                (icos_diff_ = 1 / (cos_start_ - cos_end_), infinite when blend is 0: the falloff branch is then unreachable),
 *                spot_shadow_fuzzy (shadow_fuzzy_, scales the samples of spot_soft), color (col * power) */
typedef struct yafgpu_light
{
	int32_t type, samples, cast_shadows;
	int32_t infinite;              /* directional: infinite_ (the shadow ray has no end); 0 for every other type */
	union
	{
		struct { float corner[3], c2[3], c3[3], c4[3], to_x[3], to_y[3], fnormal[3]; };      /* area */
		struct
		{	/* directional, sun, sphere */
			float direction[3], du[3], dv[3];
			float cos_angle, invpdf, pdf;
			float col_pdf[3];
			float radius, square_radius, square_radius_epsilon;
			float pad2[2];
		};
		struct
		{	/* mesh: words 4-8 of the record */
			int32_t mesh_first;        /* the scene row of the mesh's first triangle: its rows (a, eps)(e1)(e2) are contiguous from there */
			int32_t mesh_count;        /* n_tris_: its triangles, at least one */
			int32_t mesh_pool;         /* its first triangle in the light-geometry pool (yafgpu_scene_desc::light_verts) */
			int32_t double_sided;
			int32_t mesh_row;          /* filled by yafgpu_scene_create: the float at which its Pdf1D row starts in the scene's row pool,
			                              integral_, inv_integral_, func_[mesh_count], cdf_[mesh_count + 1] */
			/* portal only (word 9; a mesh light leaves it 0): power_.  For a portal mesh_first is not a scene row (its mesh has none) but,
			   filled by yafgpu_scene_create, the float (a multiple of 4) at which its triangles' records start in the scene's row pool: three
			   float4 per triangle as a scene row has them, (a, eps)(e1, material | visibility << 30)(e2, 0), then one float4 per triangle, the
			   geometric normal */
			float portal_power;
		};
		struct
		{	/* ies, ies_soft: words 14-18 of the record, behind direction, du, dv and cos_angle, which they share with the sun */
			float ies_pad[10];
			int32_t ies_first;         /* the first float of the light's tables in yafgpu_scene_desc::ies_tables: the horizontal map (ies_n_hor), the
			                              vertical map (ies_n_vert), then the table, ies_n_hor rows of ies_n_vert values.  In the scene's own copy
			                              yafgpu_scene_create moves it to where the tables lie in the scene's light-geometry pool */
			int32_t ies_n_hor, ies_n_vert;      /* at least 2 each */
			int32_t ies_type;          /* the file's photometric type: 1 C, 2 B, anything else is read like 3, A (util_ies.h:72-86) */
			float ies_max_rad;         /* max_rad_: 1 / the table's largest value, applied at lookup (util_ies.h:130) */
		};
		struct
		{	/* spot, spot_soft: words 14-16 of the record, behind direction, du, dv and cos_angle (here cos_end_), which they share with the sun */
			float spot_pad[10];
			float spot_cos_start;      /* cos_start_ = fCos__(angle * (1 - blend)): at or above it the light is not affected by the falloff */
			float spot_icos_diff;      /* icos_diff_ = 1 / (cos_start_ - cos_end_), a double quotient narrowed (light_spot.cc:42) */
			float spot_shadow_fuzzy;   /* shadow_fuzzy_: illumSample scales both of its samples by it (light_spot.cc:127) */
		};
	};
	float color[3];
	float area;                    /* mesh, portal: area_, the double sum of the float triangle areas, narrowed (light_meshlight.cc:61-68) */
	float position[3];
	float clamp_intersect;         /* background: clamp_intersect_ (Light::setClampIntersect, light_background.cc:182) */
	int32_t abs_intersect;         /* background: abs_inter_ (:178); the background factories always pass false */
} yafgpu_light;

/* The background after its factory ran on the host (background_constant.cc:51-88, background_texture.cc:33-39, :91-165).
 *   constant  color (col * power), has_ibl, shoots_caustic (always 1, background_constant.cc:69)
 *   texture   texture (index into the scene's textures), projection (0 spherical, 1 angular), power, rotation (2 * rot / 360),
 *             sin_r / cos_r (fSin__ / fCos__ of pi * rotation), has_ibl, shoots_caustic (with_caustic)
 *   gradient  has_ibl, shoots_caustic (always 1, background_gradient.cc:84); the four colours are in yafgpu_sky
 *   sunsky    has_ibl, shoots_caustic (always 1, background_sunsky.cc:220); everything else is in yafgpu_sky
 * With has_ibl the scene has exactly one YAFGPU_LIGHT_BACKGROUND light; yafgpu_scene_create builds its tables on the device. */
typedef struct yafgpu_background
{
	int32_t kind;                  /* YAFGPU_BACKGROUND_* */
	float color[3];
	float power;
	int32_t texture, projection;
	float rotation, sin_r, cos_r;
	int32_t has_ibl, shoots_caustic;
} yafgpu_background;

/* What a sky background adds to yafgpu_background, which keeps its 12 words: the constants its factory and constructor leave on the host
 * (background_gradient.cc:61-103; background_sunsky.cc:37-76, :181-264).  Read only where the background's kind is one of the two skies.
 *   gradient  horizon, zenith, horizon_ground, zenith_ground: shoriz_, szenith_, ghoriz_, gzenith_, each already times `power`
 *   sunsky    power (power_, a double parameter narrowed), from (the direction as given; it is normalised where it is used) and
 *             turbidity, kept for yafgpu_scene_create's checks; then what the constructor computes in double: theta_s, phi_s, the zenith
 *             chromaticities and luminance, and the three sets of Perez coefficients */
typedef struct yafgpu_sky
{
	float horizon[3], zenith[3], horizon_ground[3], zenith_ground[3];
	float power, from[3];
	float turbidity, pad[3];
	double theta_s, phi_s;
	double zenith_x, zenith_y, zenith_Y;
	double perez_x[5], perez_y[5], perez_Y[5];
} yafgpu_sky;

enum { YAFGPU_CAMERA_PERSPECTIVE = 0, YAFGPU_CAMERA_ARCHITECT = 1, YAFGPU_CAMERA_ANGULAR = 2, YAFGPU_CAMERA_EQUIRECTANGULAR = 3 };
/* AngularProjection (camera_angular.h); an unknown word in the ParamMap means equidistant (camera_angular.cc:109-113) */
enum { YAFGPU_ANGULAR_EQUIDISTANT = 0, YAFGPU_ANGULAR_ORTHOGRAPHIC = 1, YAFGPU_ANGULAR_STEREOGRAPHIC = 2, YAFGPU_ANGULAR_EQUISOLID_ANGLE = 3,
       YAFGPU_ANGULAR_RECTILINEAR = 4 };

/* A camera after its constructor and setAxis ran on the host.  Which fields each type reads:
 *   perspective      (camera_perspective.cc:29-74) everything up to aspect_ratio, as documented per field
 *   architect        (camera_architect.cc:29-66) the same fields; vup / vto come from its own setAxis (vup_ = aspect_ratio_ * (0, 0, -1))
 *   angular          (camera_angular.cc:29-53) position, the clip planes, resx / resy, aspect_ratio, cam_x / cam_y / cam_z, vright / vup / vto
 *                    (the unit axes; `mirrored` negates vright alone), focal_length, max_radius, circular, projection
 *   equirectangular  (camera_equirectangular.cc:29-47) as angular without the last four
 * The last two never sample a lens (Camera::sampleLense): their aperture and the other depth-of-field fields are 0. */
typedef struct yafgpu_camera
{
	float position[3], vto[3], vup[3], vright[3];
	float near_p[3], near_n[3], far_p[3], far_n[3];
	int32_t resx, resy;
	/* depth of field (camera_perspective.cc:33-54,60-74): aperture 0 = pinhole */
	float aperture, dof_distance;
	int32_t bokeh_type;            /* BokehType: 0 disk1, 1 disk2, 3 triangle, 4 square, 5 pentagon, 6 hexagon, 7 ring */
	int32_t bokeh_bias;            /* 0 none, 1 center, 2 edge */
	float bokeh_rotation;          /* degrees */
	float dof_rt[3], dof_up[3];    /* aperture * cam_x, aperture * cam_y */
	float ls[16];                  /* polygon corner table; filled by yafgpu_scene_create from bokeh_type / bokeh_rotation */
	/* for the `window` / `normal` texture coordinates (PerspectiveCamera::screenproject, Camera::getAxis) */
	float cam_x[3], cam_y[3], cam_z[3];
	float focal_distance, aspect_ratio;
	int32_t type;                  /* YAFGPU_CAMERA_*: a zeroed record is a perspective camera */
	/* angular */
	float focal_length;            /* focal_length_, by projection (camera_angular.cc:37-41) */
	float max_radius;              /* max_radius_ = max_angle / angle */
	int32_t circular;              /* circular_: a sample outside max_radius carries no ray (shootRay's wt = 0) */
	int32_t projection;            /* YAFGPU_ANGULAR_* */
} yafgpu_camera;

/* Instanced geometry (Scene::addInstance, scene.cc:1105-1130) and curve meshes (Scene::endCurveMesh, :154-281): geometry whose triangles are
 * made on the device at scene set-up.  The reference has no second tree level: a TriangleObjectInstance's
 * TriangleInstance triangles go into the one kd-tree beside every other triangle (scene.cc:797-817), so an instance is more rows of the
 * triangle, shading and texture-coordinate arrays.  With segments, yafgpu_scene_create makes ALL rows of the scene on the device, in segment
 * order (csrc/yafgpu_assemble.hip); only the base meshes and the matrices cross the bus.
 *   plain segment     rows [first, first + count) of the descriptor's own arrays (verts, tri_mat, vnormals, tri_uv, tri_orco), as they are
 *   instance segment  rows [first, first + count) of the base pools below under matrix m (row major, Matrix4 * Point3, matrix4.h:89-94)
 *   curve segment     one strand (Scene::endCurveMesh, scene.cc:154-281): points [first, first + count) of the curve point pool below,
 *                     count >= 2, extruded into a triangular prism per poly-line segment.  It makes 6 * (count - 1) + 2 rows in the
 *                     reference's order: the bottom cap, six triangles per segment, the top cap; UVs 0 -> 1 along the strand, no orco,
 *                     no vertex normals.  `first` = the first point, `count` = the number of points (not of rows), `flags` = the material
 *                     index of every row; m is not read */
enum { YAFGPU_SEGMENT_PLAIN = 0, YAFGPU_SEGMENT_INSTANCE = 1, YAFGPU_SEGMENT_CURVE = 2 };
/* what TriangleObjectInstance copied from its base when it was made (object_geom.cc:104-121) */
enum { YAFGPU_INSTANCE_SMOOTH = 1,     /* is_smooth_ || normals_exported_: TriangleInstance::getSurface reads vertex normals (triangle.cc:210-222) */
       YAFGPU_INSTANCE_ORCO = 2,       /* has_orco_: the base's orco values (triangle.cc:224-235), else the hit point */
       YAFGPU_INSTANCE_UV = 4 };       /* has_uv_: the base's UVs (triangle.cc:247-256) */
typedef struct yafgpu_segment
{
	int32_t kind;                /* YAFGPU_SEGMENT_* */
	int32_t first, count;        /* rows of the plain arrays / the base pools; a curve segment: points of the curve pool */
	uint32_t flags;              /* instance segments: YAFGPU_INSTANCE_*; curve segments: the material index */
	float m[16];                 /* obj_to_world, instance segments only */
} yafgpu_segment;
typedef struct yafgpu_instancing
{
	int32_t n_segments;          /* 0: no instanced geometry, every other field is ignored */
	const yafgpu_segment *segments;      /* in object-id order: the flattening order of Scene::update */
	/* base mesh pools, one row per base triangle */
	int32_t n_base_tris;
	const float *base_verts;     /* n_base_tris*9: the corners a, b, c */
	const int32_t *base_mat;     /* n_base_tris: the base triangle's material (triangle.cc:296) */
	const float *base_vnormals;  /* NULL or n_base_tris*9: the base's vertex normals per corner; an all-zero triple = the corner has none */
	const uint8_t *base_vn_index0;       /* with base_vnormals, n_base_tris bytes: bit c set = corner c's normal has index 0 in the base's normal
	                                        array, which TriangleInstance::getSurface's `index > 0` test sends to the geometric normal */
	const float *base_uv, *base_orco;    /* NULL or n_base_tris*6 / *9, as tri_uv / tri_orco (first word NaN: none) */
	/* curve point pool (curve segments), zeroed = none: five floats per point, x y z h s.  h and s are the two extrusion scales of
	   scene.cc:188-189 for the point's radius r, h = (float)(0.5 * r) along v and s = (float)(1.5 * r / sqrt((double)3.f)) along u.  The
	   caller computes them: r takes libm's double pow, which the device does not restate.  The tangent frame and everything after it
	   are made on the device */
	int32_t n_curve_points;
	const float *curve_points;   /* n_curve_points*5 */
} yafgpu_instancing;

typedef struct yafgpu_scene_desc
{
	int32_t n_tris;
	const float *verts;          /* n_tris*9: a,b,c */
	const int32_t *tri_mat;      /* n_tris */
	const float *vnormals;       /* NULL or n_tris*9; an all-zero triple means "use the geometric normal" */
	/* texture coordinates per triangle corner (Triangle::getSurface, triangle.cc:46-79): uv = n_tris*6 floats or NULL,
	   orco = n_tris*9 floats or NULL; only read when some material has shader nodes */
	const float *tri_uv, *tri_orco;
	int32_t n_textures; const yafgpu_texture *textures;
	uint64_t n_texels; const float *texels;      /* n_texels * 4 floats */
	int32_t n_nodes; const yafgpu_node *nodes;
	int32_t n_materials;
	const yafgpu_material *materials;
	int32_t n_lights;
	const yafgpu_light *lights;
	yafgpu_camera camera;
	int32_t build_threads;       /* host threads for the kd build; <=0: hardware concurrency */
	int32_t build_on_device;     /* kd-tree builder: 1 = on the GPU (kdtree_build_device.hip), -1 = host builder,
	                                0 = by size (GPU from 65 536 triangles on).  Both give the same query results.
	                                The environment variable YAFGPU_BUILD=device|host overrides it. */
	yafgpu_background background; /* kind 0: none.  A texture background is evaluated per escaping ray (yafgpu_render_params::background is
	                                the constant case's colour and keeps working without this record) */
	yafgpu_instancing inst;      /* instances and curves; optional, zeroed = none: then n_tris rows of the arrays above are the scene, made by the host loop as
	                                ever.  With segments the arrays above hold the plain triangles only (n_tris of them) and the scene is
	                                the segments' rows; yafgpu_tree_info::n_tris counts those */
	/* The light-geometry pool: per triangle of a mesh light the corners a, b, c as the mesh stores them (Triangle::sample reads them; the
	   scene rows hold a and the edges, and a + e1 is not bit-equal to b).  A mesh light's triangles are
	   light_verts[9 * mesh_pool .. 9 * (mesh_pool + mesh_count)), in the order of its scene rows.  yafgpu_scene_create computes the triangle
	   areas and every light's Pdf1D row from them on the device.  Zeroed = no mesh light */
	int32_t n_light_tris;
	const float *light_verts;    /* n_light_tris*9 */
	/* A portal light's triangles have no scene row to take a material from: per triangle of the pool its material index (of `materials`),
	   which a portal's triangle records carry with that material's visibility.  Read for the portals' ranges only; null when the scene has
	   no portal light */
	const int32_t *light_tri_mat; /* n_light_tris */
	/* The measured tables of the IES lights (yafgpu_light::ies_first), one float pool: per light its horizontal map, its vertical map (both
	   strictly increasing, in degrees) and its table, row-major by horizontal angle.  Zeroed = no IES light */
	int32_t n_ies_floats;
	const float *ies_tables;     /* n_ies_floats */
	yafgpu_sky sky;              /* the constants of a gradient or sunsky background; read only with background.kind 4 or 5 */
} yafgpu_scene_desc;

typedef struct yafgpu_render_params
{
	int32_t integrator;            /* YAFGPU_INTEGRATOR_* */
	int32_t path_samples, bounces, rr_min_bounces, no_recursive, bg_transp, bg_transp_refract;
	int32_t width, height, xstart, ystart;
	int32_t aa_minsamples;
	float aa_pixelwidth;           /* reconstruction filter width in pixels (AA_pixelwidth) */
	int32_t filter_type;           /* YAFGPU_FILTER_*: box | mitchell | gauss | lanczos (ImageFilm::FilterType, imagefilm.cc:155-163) */
	int32_t tile_size;
	uint32_t base_sampling_offset;
	int32_t shadow_bias_auto; float shadow_bias;
	int32_t min_raydist_auto; float min_raydist;
	float aa_light_sample_multiplier;
	float background[3]; int32_t has_background;
	/* pixel-tile sharding across GPUs: tile t is rendered iff t % shard_count == shard_index */
	int32_t shard_index, shard_count;
	/* one pass of the multi-pass schedule (TiledIntegrator::renderPass, integrator_tiled.cc:261-307); all zero for a
	   single-pass render.  aa_minsamples is the sample count of THIS pass. */
	int32_t multi_pass;            /* AA_passes > 1: sub-pixel positions from riVdC / riS (integrator_tiled.cc:394-398) */
	uint32_t pass_offset;          /* samples per pixel taken by the earlier passes (renderPass's `offset`) */
	int32_t accumulate;            /* add to the planes instead of starting from zero */
	float aa_clamp_samples;        /* ImageFilm::addSample clampProportionalRgb (imagefilm.cc:975); 0 = off */
	int32_t transp_shad;           /* tr_shad_: shadow rays are filtered by transparent materials instead of blocked
	                                  (TriKdTree::intersectTs, kdtree_triangle.cc:983-1162) */
	int32_t shadow_depth;          /* s_depth_: more distinct transparent surfaces than this along a shadow ray block it; at most 8 */
	int32_t raydepth;              /* r_depth_ of recursiveRaytrace (integrator_montecarlo.cc:791): levels of perfect specular
	                                  reflection / filtered transmission followed from a camera hit; at most 7 */
	int32_t serial_replay;         /* 1: replay the reference's serial state as its single-threaded render consumes it — the per-tile
	                                  MWC stream of Russian roulette (integrator_tiled.cc:319, integrator_path_tracer.cc:282-288) and
	                                  the estimateOneDirectLight counter (integrator_montecarlo.cc:62-76) — with a record pass, a scan
	                                  in the reference's sample order and the final pass (yafgpu_wavefront.h, WfArgs::replay).
	                                  0: per-sample streams (same distribution, not the reference's pixels). */
	const int32_t *tile_rand;      /* HOST pointer, one value per tile of the frame (row-major tile order): the libc rand() value
	                                  TiledIntegrator::renderTile seeds that tile's Random with in THIS pass; NULL = 0 for all */
	const uint8_t *resample_mask;  /* HOST pointer, width*height bytes, row-major in window coordinates: the pixels that
	                                  get samples in this pass (ImageFilm::doMoreSamples, imagefilm.cc:917-920); NULL = all */
	int32_t trace_caustics;        /* PathIntegrator::trace_caustics_ (integrator_path_tracer.cc:85): caustic_type "path" — the factory's default when the
	                                  parameter is absent — or "both": after a bounce through a specular, glossy or filter lobe the next vertex shows its
	                                  lights and adds its emission (:252-253, :290).  0 = caustic_type "none" */
	/* Ambient occlusion of the direct lighting integrator (DirectLightIntegrator::integrate, integrator_direct_light.cc:145;
	   MonteCarloIntegrator::sampleAmbientOcclusion, integrator_montecarlo.cc:1030-1088): at every hit with a diffuse component,
	   ao_samples shadow rays of length ao_distance in directions drawn from the material's BSDF.  Read only where integrator is
	   YAFGPU_INTEGRATOR_DIRECT; ao_samples in [1, 4095], and at most 254 lights beside it (yafgpu_wavefront.h, pack_dlc) */
	int32_t do_ao, ao_samples;
	float ao_distance, ao_color[3];
} yafgpu_render_params;

/* Scene::setAntialiasing (scene.cc:761-778; defaults environment.cc:682-695) */
typedef struct yafgpu_aa_schedule
{
	int32_t passes, inc_samples;
	float threshold, resampled_floor;
	float sample_multiplier_factor, light_sample_multiplier_factor;
	int32_t detect_color_noise;
	int32_t dark_detection_type;   /* 0 none, 1 linear, 2 curve */
	float dark_threshold_factor;
	int32_t variance_edge_size, variance_pixels;
	/* libc state behind the tile seeds (used with yafgpu_render_params::serial_replay): srand(rand_srand) by the last
	   Material / ObjectGeometric constructor (material.cc:56, object_geom.cc:42), rand_skip values consumed by its colour
	   loop since; then one rand() per tile per pass that runs.  rand_srand < 0: every tile draws 0. */
	int32_t rand_srand, rand_skip;
	/* A resumed render (session__.renderResumed(), integrator_tiled.cc:196-203; read by yafgpu_render_passes_to_host alone): the film
	   so far instead of the first pass.  The first pass then launches no path work and counts no camera samples (resampled[0] = 0) but
	   still consumes its block of tile seeds, as renderTile does with zero samples (:319); the adaptive passes 1 .. passes - 1 follow
	   on the seeded film with their sample numbers starting at resume_sampling_offset.  passes <= 1: the films are only combined. */
	const float *resume_film;      /* HOST pointer, [height][width][5] floats, or NULL: an ordinary render */
	uint32_t resume_sampling_offset;       /* samples per pixel the film holds (renderPass's `offset` of the pass that follows) */
	/* More films to add to resume_film on the device, in the order they are handed out (ImageFilm::imageFilmLoadAllInFolder's
	   col += , weight += in float32, starting from a zero film, imagefilm.cc:1520-1531): called until it returns 0; it writes the next
	   film, n_floats = height * width * 5 values, into dst (host memory) and returns 1, or a negative number on failure, which fails
	   the render.  NULL: resume_film is the only film, and goes into the planes as it is. */
	int (*resume_next)(void *user, float *dst, uint64_t n_floats);
	void *resume_user;
} yafgpu_aa_schedule;

typedef struct yafgpu_counters   /* device atomics, accumulated per launch */
{
	uint64_t rays_closest, rays_shadow, interior_steps, leaves, tri_tests, camera_samples, restarts;
	uint64_t wave_rounds;   /* YAFGPU_STATS only: node-step rounds executed by waves | triangle rounds << 32 (SIMT efficiency of the traversal) */
} yafgpu_counters;

typedef struct yafgpu_tree_info
{
	uint32_t n_nodes, n_leaf_refs, max_depth, n_tris;
	double build_seconds, upload_seconds;
	uint64_t device_bytes;
} yafgpu_tree_info;

typedef struct yafgpu_scene yafgpu_scene_t;

/* all functions return 0 on success, a negative code on failure; yafgpu_last_error() describes it */
const char *yafgpu_last_error(void);
int yafgpu_device_count(void);
int yafgpu_set_device(int device);

int yafgpu_scene_create(const yafgpu_scene_desc *desc, yafgpu_scene_t **out);
void yafgpu_scene_destroy(yafgpu_scene_t *scene);
int yafgpu_scene_info(const yafgpu_scene_t *scene, yafgpu_tree_info *info);

/* bytes of one plane set: YAFGPU_FILM_PLANES*height*width*YAFGPU_FILM_CHANNELS floats */
uint64_t yafgpu_planes_bytes(int32_t width, int32_t height);

/* Render every tile of this shard.  d_planes: device pointer to yafgpu_planes_bytes() bytes (zeroed by
 * the call); d_counters: device pointer to a yafgpu_counters (may be NULL); stream: hipStream_t or NULL.
 * Asynchronous on `stream`. */
int yafgpu_render_tiles(yafgpu_scene_t *scene, const yafgpu_render_params *rp, float *d_planes,
                        yafgpu_counters *d_counters, void *stream);

/* d_film[h][w][5] = own + right(x-1) + down(y-1) + diag(x-1,y-1), in that fixed order */
int yafgpu_film_combine(const float *d_planes, float *d_film, int32_t width, int32_t height, void *stream);

/* The output stage (yafgpu_output.hip): a film [height][width][5] becomes the packed pixels of an image, one pixel per lane.  Per
 * pixel, in ImageFilm::flush's order for the combined pass (imagefilm.cc:737-772): Pixel::normalized, clampRgb0,
 * colorSpaceFromLinearRgb, alpha clamped to [0, 1]; then one of three packings:
 *   YAFGPU_IMAGE_FLOAT  four floats r g b a, what a ColorOutput's putPixel receives (16 bytes a pixel)
 *   YAFGPU_IMAGE_RGBA8  clampRgba01 and (uint8_t)(c * 255.f), a truncation, bytes r g b a; alpha = 0 makes the alpha byte 255
 *   YAFGPU_IMAGE_RGBE   RgbePixel::operator=(const Rgb &) (imagehandler_util_hdr.h:52-71), bytes r g b e
 * The image is image_width x image_height pixels, rows outermost; the film lands at (border_x, border_y) and every other pixel is zero.
 * What the reference's casts leave undefined is defined: a NaN channel packs to the byte 0, and a pixel whose largest colour channel is
 * not finite packs to four zero bytes in RGBE. */
#define YAFGPU_IMAGE_FLOAT 0
#define YAFGPU_IMAGE_RGBA8 1
#define YAFGPU_IMAGE_RGBE 2
typedef struct yafgpu_image_desc
{
	int32_t width, height;         /* the film: the render window */
	int32_t color_space;           /* 0 sRGB, 1 XYZ, 2 LinearRGB, 3 Raw_Manual_Gamma */
	float gamma;                   /* Raw_Manual_Gamma alone reads it */
	int32_t alpha;                 /* YAFGPU_IMAGE_RGBA8 alone reads it */
	int32_t format;                /* YAFGPU_IMAGE_* */
	int32_t image_width, image_height, border_x, border_y;
} yafgpu_image_desc;
/* bytes of an image of that format and size; 0 for a size or a format out of range */
uint64_t yafgpu_image_bytes(int32_t format, int32_t width, int32_t height);
/* d_film and d_image are device pointers (d_image: yafgpu_image_bytes of the image's size, aligned to 16 bytes); one launch,
 * asynchronous on `stream`.  Sizes and the border are checked before anything is launched. */
int yafgpu_film_to_image(const float *d_film, const yafgpu_image_desc *desc, void *d_image, void *stream);
/* The same for the film the scene's render targets hold after yafgpu_render_to_host / yafgpu_render_passes_to_host (desc->width and
 * height must be that render's), with no upload: converted on the device, downloaded into h_image (host memory), synchronised.
 * -13 when the scene holds no finished film of that size (nothing rendered yet, or a render that failed). */
int yafgpu_scene_film_to_image(yafgpu_scene_t *scene, const yafgpu_image_desc *desc, void *h_image);

/* Convenience: allocate, render, combine, copy the film to host memory, synchronise. */
/* TiledIntegrator::render (integrator_tiled.cc:116-258): pass 0 with rp->aa_minsamples samples, then aa->passes - 1
   adaptive passes; between passes ImageFilm::nextPass (imagefilm.cc:270-480) picks the pixels to resample from the
   film so far.  aa == NULL or aa->passes <= 1: one pass.  resampled[] (optional, aa->passes entries) receives the
   number of pixels each pass sampled. */
int yafgpu_render_passes_to_host(yafgpu_scene_t *scene, const yafgpu_render_params *rp, const yafgpu_aa_schedule *aa,
                                 float *h_film, yafgpu_counters *h_counters, int32_t *resampled);
int yafgpu_render_to_host(yafgpu_scene_t *scene, const yafgpu_render_params *rp, float *h_film, yafgpu_counters *h_counters);

/* Ray batches (host pointers): rays = n*8 floats {from.xyz, dir.xyz, tmin, tmax}; closest-hit writes
 * tri (int32, -1 = miss), t, and barycentrics b0,b1,b2 (n*3); any-hit writes 0/1 into shadowed. */
int yafgpu_trace_closest(yafgpu_scene_t *scene, int32_t n, const float *rays, int32_t *tri, float *t, float *bary);
int yafgpu_trace_shadow(yafgpu_scene_t *scene, int32_t n, const float *rays, int32_t *shadowed);
/* The traversal kernels' queue schedule, for tests.  yafgpu_trace_reservation: the entries a wave reserves with `seen` of `n` queue
 * entries handed out and `waves` waves in the launch, by the rule the library was built with.  yafgpu_trace_schedule: info[0..5] = the
 * smallest and the largest reservation, the divisor D, whether the sizes shrink, whether a wave's first range is static, and the
 * waves per workgroup, as built; info[6], info[7] = the workgroups of this process's last closest-hit and any-hit traversal launch,
 * of a render or of a ray batch (0: none yet), where the switch YAFGPU_TRACE_GRID_CAP shows. */
uint32_t yafgpu_trace_reservation(uint32_t n, uint32_t seen, uint32_t waves);
void yafgpu_trace_schedule(uint32_t info[8]);

/* Per-kernel device timing of the NEXT render pass (HIP events around every launch on the pass's own
 * stream; the pass then synchronises after each launch, so it is a measurement mode, not a fast path).
 * slots: 0 closest-hit traversal, 1 any-hit traversal, 2 shading, 3 other (ray generation, film). */
int yafgpu_set_profiling(yafgpu_scene_t *scene, int32_t enable);
/* Pass pipelining: consecutive yafgpu_render_tiles calls whose passes do not depend on each other's film (no resample mask, no serial-state
 * replay, no recursion, one chunk) run their path work on two internal streams with a buffer set each, so that one pass's launch tails are
 * filled by the other's launches; everything the caller sees (the planes, the counters) is still written on the caller's stream, in call
 * order.  mode -1 (default): on for passes of up to 12 Mi paths, where it pays (an eighth of the metric frame: +18 %); 0: off; 1: on. */
int yafgpu_scene_set_pass_pipelining(yafgpu_scene_t *scene, int32_t mode);
/* glibc's rand() after srand(seed) (TYPE_3 additive feedback generator, restated; pinned against libc in the tests):
 * out[k] = the k-th value.  The tile seeds of a render are drawn from it (integrator_tiled.cc:319). */
void yafgpu_glibc_rand(uint32_t seed, int32_t count, int32_t *out);
/* Scene::abort (scene.cc:75-89): the render entry points poll *flag between wavefront chunks and between passes and
 * return -30 ("aborted") once it is non-zero.  The flag stays owned by the caller; NULL detaches it. */
int yafgpu_scene_set_abort_flag(yafgpu_scene_t *scene, const volatile int32_t *flag);
/* Multi-pass (adaptive) anti-aliasing on a sharded frame: the noise detection between passes (integrator_tiled.cc:136-258) reads
 * every pixel, other ranks' tiles included.  With an exchange function attached, yafgpu_render_passes_to_host hands it a COPY of
 * this rank's four splat planes (device memory, n_floats values) after every pass that is followed by a detection step; the
 * function sums the copies over all ranks in place (an all-reduce: RCCL over xGMI) and returns 0.  Every plane element is
 * written by exactly one rank, so the sums are exact (x + 0) and every rank derives the single-GPU render's resample mask.
 * The rank's own planes, and the film it returns at the end, stay its own share.
 * The same function carries the reference's serial light counter across ranks (path tracing with more than one light,
 * estimateOneDirectLight's correlative_sample_number_, integrator_montecarlo.cc:62-76): once per pass every rank — with or without
 * tiles of its own — hands it a table of 2 x (tiles of the frame) floats holding its own tiles' call counts; see DESIGN.md §6. */
typedef int (*yafgpu_exchange_fn)(void *user, float *d_values, uint64_t n_floats);
int yafgpu_scene_set_exchange(yafgpu_scene_t *scene, yafgpu_exchange_fn fn, void *user);
int yafgpu_get_profile(const yafgpu_scene_t *scene, double ms[4], uint64_t launches[4]);

/* Component probe for tests: evaluates device-side leaf functions (fast-math, QMC, camera, lights,
 * material eval/pdf/sample) on n items of n_in floats each, writing n_out floats each; `op` selects the
 * function (see probe_kernel in yafgpu_device.hip).  Lets the device code be pinned against the
 * reference's own golden vectors independently of any render. */
int yafgpu_probe(yafgpu_scene_t *scene, int32_t op, int32_t n, const float *in, int32_t n_in, float *out, int32_t n_out);

/* Host-only kd-tree build (no device needed): the builder Scene::update would run (scene.cc:818 ->
 * TriKdTree ctor, kdtree_triangle.cc:76-157), exposed so that host tests can check the tree the
 * kernels will walk.  nodes = n_nodes*2 uint32 (kdtree_build.h layout), refs = n_leaf_refs uint32. */
typedef struct yafgpu_kdtree yafgpu_kdtree_t;
/* the same on the GPU (needs a device); NULL on failure, yafgpu_last_error() says why */
yafgpu_kdtree_t *yafgpu_kdtree_build_device(const float *verts, int32_t n_tris);
yafgpu_kdtree_t *yafgpu_kdtree_build(const float *verts, int32_t n_tris, int32_t threads);
void yafgpu_kdtree_info(const yafgpu_kdtree_t *tree, yafgpu_tree_info *info);
void yafgpu_kdtree_get(const yafgpu_kdtree_t *tree, uint32_t *nodes, uint32_t *refs, float bound6[6]);
/* The treelet layout the traversal kernels walk (kdtree_build.h, TreeletLayout), built from n_nodes nodes as yafgpu_kdtree_get
 * returns them.  *n_words / *n_leaves: room of words / leaves on entry (either may be NULL to ask for the sizes only), the sizes
 * on return.  inline_leaves = 0 sends every non-empty leaf to the escape array.  0, or -2 when the tree is too large. */
int32_t yafgpu_kdtree_treelets(const uint32_t *nodes, uint32_t n_nodes, int32_t inline_leaves, uint32_t *words, uint32_t *n_words,
                               uint32_t *leaves, uint32_t *n_leaves, uint32_t *root);
/* Where the traversal's own copy of the triangle records keeps every triangle (kdtree_build.h, tri_order): pos[t] = the rank of
 * triangle t's first occurrence in the n_refs leaf references as yafgpu_kdtree_get returns them, unreferenced triangles behind the
 * referenced ones in id order.  pos has room for n_tris values.  (A scene created with YAFGPU_TRI_ORDER=id takes the identity.) */
void yafgpu_kdtree_tri_order(const uint32_t *refs, uint32_t n_refs, uint32_t n_tris, uint32_t *pos);
void yafgpu_kdtree_destroy(yafgpu_kdtree_t *tree);

/* kd-tree built on the host, downloadable for inspection/tests: nodes = n_nodes*2 uint32, refs = n_leaf_refs uint32 */
int yafgpu_scene_get_tree(const yafgpu_scene_t *scene, uint32_t *nodes, uint32_t *refs, float bound6[6]);

#ifdef __cplusplus
}
#endif
#endif
