/* yafaray_c_api.h — the drop-in boundary: libYafaRay's scene/render API as a C ABI.
 *
 * The reference snapshot has no C API; its public surface is the C++ class yafaray4::Interface
 * (include/interface/interface.h:48-139, src/interface/interface.cc) reached through the single
 * C-linkage factory getYafray__() (interface.cc:451-457).  This header flattens that class 1:1 —
 * one function per Interface method, same name, same argument meaning, the object as first
 * parameter — so a binding written against Interface ports by renaming.  Each declaration cites
 * the method it replaces.  Error convention of the reference is kept: bool results (0 = wrong
 * state / missing object), NULL from failed create*, no exceptions; additionally
 * yafaray_getLastError() returns the diagnostic the reference would have logged.
 *
 * Scope: scenes of type "triangle"; materials shinydiffusemat / glossy(as_diffuse) /
 * coated_glossy(as_diffuse) / glass / mirror / light_mat; lights arealight / pointlight; camera perspective (with depth of
 * field); background constant; integrators pathtracing / directlighting; volume integrator none; image files tga / hdr / png written
 * from the device film (createImageHandler + createImageOutput).  Every method of
 * Interface has a function here: what lies outside the scope fails loudly (0 / NULL + yafaray_getLastError) at the call
 * or at render time — nothing falls back to a CPU path, and nothing is silently dropped.
 */
#ifndef YAFARAY_C_API_H
#define YAFARAY_C_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int yafaray_bool_t;
typedef struct yafaray_interface yafaray_interface_t;
/* borrowed handles, owned by the interface until clearAll (environment.h:85-95) */
typedef struct yafaray_material yafaray_material_t;
typedef struct yafaray_light yafaray_light_t;
typedef struct yafaray_texture yafaray_texture_t;
typedef struct yafaray_camera yafaray_camera_t;
typedef struct yafaray_background yafaray_background_t;
typedef struct yafaray_integrator yafaray_integrator_t;

/* ColorOutput (include/output/output.h:38-51) as a callback table; any member may be NULL.
 * putPixel receives linear RGBA of the "combined" pass, x/y relative to the render window. */
typedef struct yafaray_output
{
	void *user;
	yafaray_bool_t (*putPixel)(void *user, int num_view, int x, int y, float r, float g, float b, float a);
	void (*flush)(void *user, int num_view);
	void (*flushArea)(void *user, int num_view, int x0, int y0, int x1, int y1);
	void (*highlightArea)(void *user, int num_view, int x0, int y0, int x1, int y1);
} yafaray_output_t;

/* ProgressBar (include/common/monitor.h:29-44) */
typedef struct yafaray_progress
{
	void *user;
	void (*init)(void *user, int total_steps);
	void (*update)(void *user, int steps);
	void (*done)(void *user);
	void (*setTag)(void *user, const char *text);
} yafaray_progress_t;

/* Interface::Interface / ~Interface, interface.cc:85-103 ; getYafray__ :451-457 */
yafaray_interface_t *yafaray_createInterface(void);
void yafaray_destroyInterface(yafaray_interface_t *yi);
const char *yafaray_getLastError(const yafaray_interface_t *yi);
const char *yafaray_getVersion(void);                                            /* interface.h:117 */

/* scene state machine — Interface::startScene .. endGeometry, interface.cc:113-219 */
yafaray_bool_t yafaray_startScene(yafaray_interface_t *yi, int type);            /* interface.h:103 */
yafaray_bool_t yafaray_startGeometry(yafaray_interface_t *yi);                   /* :54 */
yafaray_bool_t yafaray_endGeometry(yafaray_interface_t *yi);                     /* :55 */
unsigned int yafaray_getNextFreeId(yafaray_interface_t *yi);                     /* :60 */
yafaray_bool_t yafaray_startTriMesh(yafaray_interface_t *yi, unsigned int id, int vertices, int triangles,
                                    yafaray_bool_t has_orco, yafaray_bool_t has_uv, int type, int obj_pass_index); /* :61 */
yafaray_bool_t yafaray_endTriMesh(yafaray_interface_t *yi);                      /* :64 */
int yafaray_addVertex(yafaray_interface_t *yi, double x, double y, double z);    /* :66 */
void yafaray_addNormal(yafaray_interface_t *yi, double nx, double ny, double nz);/* :68 */
yafaray_bool_t yafaray_addTriangle(yafaray_interface_t *yi, int a, int b, int c, const yafaray_material_t *mat); /* :69 */
yafaray_bool_t yafaray_smoothMesh(yafaray_interface_t *yi, unsigned int id, double angle); /* :72 */
yafaray_bool_t yafaray_startTriMeshPtr(yafaray_interface_t *yi, unsigned int *id, int vertices, int triangles,
                                       yafaray_bool_t has_orco, yafaray_bool_t has_uv, int type, int obj_pass_index); /* :63 */
int yafaray_addVertexWithOrco(yafaray_interface_t *yi, double x, double y, double z, double ox, double oy, double oz); /* :67, the orco overload of addVertex */
int yafaray_addUv(yafaray_interface_t *yi, float u, float v);                    /* :71 */
yafaray_bool_t yafaray_addTriangleWithUv(yafaray_interface_t *yi, int a, int b, int c, int uv_a, int uv_b, int uv_c,
                                         const yafaray_material_t *mat);          /* :70, the UV overload of addTriangle */
/* Scene::addInstance (scene.cc:1105-1130): one more object, under an id of its own from getNextFreeId, whose triangles are the base
 * mesh's under obj_to_world (row major).  Any mesh can be the base, flagged BASEMESH (type & 0x0200) or not; no geometry-state check.  The
 * instance keeps the base's has_orco / has_uv / is_smooth / normals_exported flags AS THEY ARE NOW (object_geom.cc:104-121): a base
 * smoothed later leaves it unsmoothed.  Refused, with the cause in getLastError: a base id that names no mesh, a null matrix, a matrix
 * with a non-finite entry, a base that is itself an instance.  The triangles are made on the device at scene set-up. */
yafaray_bool_t yafaray_addInstance(yafaray_interface_t *yi, unsigned int base_object_id, const float *obj_to_world_16); /* :73 */
/* extension (test support): what addInstance stored, in object-id order: up to max_instances records of 22 32-bit words: own id, base
 * id, has_orco, has_uv, is_smooth, normals_exported (the flags as they stood at the call), then the 16 matrix floats.  Returns the
 * number of instances */
int yafaray_getInstances(yafaray_interface_t *yi, void *out, int max_instances);
/* Curve meshes (Scene::startCurveMesh / endCurveMesh, scene.cc:133-281): a strand of hair, fur or grass as a poly-line with a root radius
 * (strand_start), a tip radius (strand_end) and a shape exponent (strand_shape).  The reference extrudes every point into a triangular
 * cross-section and fills a prism per segment, 6 * (n - 1) + 2 triangles with UVs that run 0 -> 1 along the strand, into an ordinary
 * TriangleObject (UVs, no orco, visible, no base mesh).  Here the points are kept and the triangles are made on the device at scene set-up,
 * in the reference's order and arithmetic; the radii are computed at endCurveMesh with the host's libm, as the reference does.
 *   startCurveMesh  only between startGeometry and endGeometry and outside any open object; opens an object of its own under `id` (a mesh
 *                   or an instance that had the id is replaced).  `vertices` is a reservation hint.
 *   in between      addVertex only; addVertexWithOrco, addNormal, addUv, addTriangle*, addTriangles and endTriMesh are refused.
 *   endCurveMesh    refused, and the object dropped, for a null material, fewer than two points, a non-finite point or parameter, or
 *                   parameters that give a non-finite radius (a shape below -1 raises 0 to a negative power).
 * smoothMesh on a curve's id and addInstance with a curve as its base are refused: a curve has no stored faces. */
yafaray_bool_t yafaray_startCurveMesh(yafaray_interface_t *yi, unsigned int id, int vertices, int obj_pass_index);       /* :62 */
yafaray_bool_t yafaray_endCurveMesh(yafaray_interface_t *yi, const yafaray_material_t *mat, float strand_start, float strand_end, float strand_shape); /* :65 */
/* extension: n_curves strands in one call, curve k with n_points[k] points taken in turn from the packed xyz floats of `points`, all with
 * one material and one set of strand parameters.  Defined as the loop of getNextFreeId / startCurveMesh / addVertex per point /
 * endCurveMesh, which it stops at the first refusal; ids (NULL or n_curves entries) receives the object ids */
yafaray_bool_t yafaray_addCurves(yafaray_interface_t *yi, int n_curves, const int *n_points, const float *points, const yafaray_material_t *mat,
                                 float strand_start, float strand_end, float strand_shape, unsigned int *ids);
/* extension (test support): what endCurveMesh stored, in object-id order, as a stream of 32-bit words.  Per curve: id, point count n,
 * material index, then the floats strand_start, strand_end, strand_shape, then per point x y z h s, where h = (float)(0.5 * r) and
 * s = (float)(1.5 * r / sqrt((double)3.f)) scale the two frame vectors of the extrusion (scene.cc:188-189).  Whole records are written
 * while they fit into max_words; *n_words (NULL or one int) receives what all of them take.  Returns the number of curves */
int yafaray_getCurves(yafaray_interface_t *yi, void *out, int max_words, int *n_words);
/* extension (test support): the per-triangle-corner normals smoothMesh computed, n_tris*9 floats; an all-zero triple = geometric normal */
yafaray_bool_t yafaray_getMeshCornerNormals(yafaray_interface_t *yi, unsigned int id, float *out, int n_floats);
/* extension (test support): the scene's enabled lights in Scene::addLight order, as the device gets them: up to max_lights
 * yafgpu_light records (include/yafgpu.h, 136 bytes each) into out; returns how many lights the scene has */
int yafaray_getLights(yafaray_interface_t *yi, void *out, int max_lights);
/* extension (test support): the yafgpu_background record (include/yafgpu.h, 12 words) createBackground made under `name`, as the
 * device scene would get it; false when there is no such background */
yafaray_bool_t yafaray_getBackground(yafaray_interface_t *yi, const char *name, void *out);
/* extension (test support): the yafgpu_sky record (include/yafgpu.h, 240 bytes: 20 float words, then 20 doubles) createBackground made
 * under `name` beside its yafgpu_background: a gradientback's colours or a sunsky's constants, zeros for every other type; false when
 * there is no such background */
yafaray_bool_t yafaray_getSky(yafaray_interface_t *yi, const char *name, void *out);
/* extension (test support): the yafgpu_camera record (include/yafgpu.h, 69 words) createCamera made under `name`, as the device scene
 * would get it — but for the bokeh corner table `ls`, which yafgpu_scene_create fills; false when there is no such camera */
yafaray_bool_t yafaray_getCamera(yafaray_interface_t *yi, const char *name, void *out);
/* extension (test support): the ambient occlusion settings createIntegrator parsed for the integrator `name` (do_AO, AO_samples,
 * AO_distance narrowed to float, AO_color as three floats); any out pointer may be NULL; false when there is no such integrator */
yafaray_bool_t yafaray_getIntegratorAO(yafaray_interface_t *yi, const char *name, int *do_ao, int *samples, float *distance, float *color3);
/* extension (test support): what MaskMaterial::factory's restatement parsed for the mask_mat `name`.  out8 receives eight 32-bit words:
 * the indices of material1 and material2 in creation order, threshold_ (a float's bits), the mask node's slot among the mask's nodes,
 * how many nodes that is, receive_shadows, visibility (0 normal, 1 no_shadows, 2 shadow_only, 3 invisible) and the union of both
 * sub-materials' bsdf flags; false when there is no such material or it is no mask_mat */
yafaray_bool_t yafaray_getMaskMaterial(yafaray_interface_t *yi, const char *name, void *out8);
/* An ieslight's parsed file (a test hook for the parser): the photometric type, the counts of horizontal and vertical angles (after a
 * single horizontal angle was doubled), max_rad_ and the largest vertical angle in radians; then up to n_floats floats of the horizontal
 * map, the vertical map and the table, row-major by horizontal angle.  Any pointer may be null. */
yafaray_bool_t yafaray_getIesLight(yafaray_interface_t *yi, const char *name, int *type, int *n_hor, int *n_vert, float *max_rad, float *max_v_angle, float *out, int n_floats);
/* extension (test support): what BlendMaterial::factory's restatement parsed for the blend_mat `name`.  out10 receives ten 32-bit words:
 * the indices of material1 and material2 in creation order, blend_val_ (a float's bits), whether a shader node drives the blend (0 / 1),
 * that node's slot among the blend's nodes (-1 without one), how many nodes that is, receive_shadows, visibility (0 normal, 1 no_shadows,
 * 2 shadow_only, 3 invisible), the union of both sub-materials' bsdf flags and additional_depth_, the larger of theirs; false when there
 * is no such material or it is no blend_mat */
yafaray_bool_t yafaray_getBlendMaterial(yafaray_interface_t *yi, const char *name, void *out10);
/* extension (test support): the material table as the device scene would get it: the materials in creation order, then for every
 * mask_mat the two hidden clones of its sub-materials it picks from, and for every blend_mat the two it mixes.  Up to max_materials yafgpu_material records (include/yafgpu.h,
 * 384 bytes each) into out; returns how many records the table has */
int yafaray_getMaterialTable(yafaray_interface_t *yi, void *out, int max_materials);
/* extension (not in the reference): bulk form of addVertex/addTriangle for large meshes;
 * verts = n_verts*3 floats, indices = n_tris*3 ints, one material for all triangles */
yafaray_bool_t yafaray_addTriangles(yafaray_interface_t *yi, int n_verts, const float *verts, int n_tris, const int *indices,
                                    const yafaray_material_t *mat);

/* ParamMap builders — interface.cc:221-310 */
void yafaray_paramsSetPoint(yafaray_interface_t *yi, const char *name, double x, double y, double z);   /* :76 */
void yafaray_paramsSetString(yafaray_interface_t *yi, const char *name, const char *s);                 /* :77 */
void yafaray_paramsSetBool(yafaray_interface_t *yi, const char *name, yafaray_bool_t b);                /* :78 */
void yafaray_paramsSetInt(yafaray_interface_t *yi, const char *name, int i);                            /* :79 */
void yafaray_paramsSetFloat(yafaray_interface_t *yi, const char *name, double f);                       /* :80 */
void yafaray_paramsSetColor(yafaray_interface_t *yi, const char *name, float r, float g, float b, float a); /* :81 */
void yafaray_paramsSetColorArray(yafaray_interface_t *yi, const char *name, const float *rgb, yafaray_bool_t with_alpha); /* :82 */
void yafaray_paramsSetMatrix(yafaray_interface_t *yi, const char *name, const float *m16, yafaray_bool_t transpose);   /* :83, :85 (paramsSetMemMatrix): 16 floats, row major */
void yafaray_paramsSetMatrixD(yafaray_interface_t *yi, const char *name, const double *m16, yafaray_bool_t transpose); /* :84, :86 */
/* Interface::setInputColorSpace (:127; interface.cc:292-301): the colour space paramsSetColor reads its arguments in
 * ("sRGB" | "XYZ" | "LinearRGB" | "Raw_Manual_Gamma"; converted to linear RGB on entry, interface.cc:247-252) */
void yafaray_setInputColorSpace(yafaray_interface_t *yi, const char *color_space_string, float gamma_val);
void yafaray_paramsClearAll(yafaray_interface_t *yi);                                                   /* :87 */
void yafaray_paramsStartList(yafaray_interface_t *yi);                                                  /* :88 */
void yafaray_paramsPushList(yafaray_interface_t *yi);                                                   /* :89 */
void yafaray_paramsEndList(yafaray_interface_t *yi);                                                    /* :90 */

/* RenderEnvironment factories — interface.cc:312-372; dispatch on the "type" string exactly like
 * Material::factory (src/material/material.cc:36-52), Light::factory (src/light/light.cc:36-51),
 * Camera::factory (src/camera/camera.cc:34-44), Integrator::factory (src/integrator/integrator.cc:36-57) */
/* createLight: arealight, pointlight, directionallight, sunlight and spherelight (light_area.cc, light_point.cc, light_directional.cc,
 * light_sun.cc, light_sphere.cc factories); every other type, and photon_only lights, are refused with a diagnostic.  A sphere light's
 * `object` is accepted and changes nothing: the mesh it names renders as the light-material geometry it is.
 * meshlight (light_meshlight.cc): object, color, power, samples, double_sided, light_enabled, cast_shadows; with_caustic / with_diffuse are
 * read and dropped.  Without an `object` it is refused here.  The mesh is looked up at prepareRender (MeshLight::init runs at scene update),
 * so the light may be created before or after its mesh; prepareRender refuses an object that names no mesh, a curve mesh or an instance
 * (their triangles exist on the device only), a mesh that is not rendered, one with no triangles and one whose total area is zero or not
 * finite.  The mesh stays ordinary scene geometry with the material it has.  yafaray_getLights then shows the rows the light resolved to and
 * its area_.
 * bgPortalLight (light_background_portal.cc): object, samples, power (a float), light_enabled, cast_shadows; with_caustic / with_diffuse are
 * read and dropped; no color and no double_sided.  Without an `object` it is refused here.  Its mesh must be a plain triangle mesh created
 * invisible (startTriMesh type bit 0x0100): BackgroundPortalLight::init hides the mesh, so its triangles are no scene geometry and live
 * with the light.  prepareRender refuses a scene with no background, an object that names no mesh, a curve mesh or an instance, the base of
 * instances, a visible mesh, one with no triangles and one whose total area is zero or not finite.  yafaray_getLights then shows the
 * light's triangles in the light-geometry pool and its area_.
 * ieslight (light_ies.cc): from, to, color, power, file, samples (16), soft_shadows (false), light_enabled, cast_shadows; cone_angle,
 * with_caustic and with_diffuse are read and dropped.  `file` is an IES photometric file, looked up like a texture's filename; it is parsed
 * here, and a file that is missing, cut off, malformed or larger than 4096 angles a side is refused with its cause.  Without soft_shadows
 * the light is a Dirac light with a table lookup, with it a sampled light of `samples` samples that cannot be intersected.  Without a
 * `file` it is refused.
 * spotlight (light_spot.cc): from, to, color, power, cone_angle (45: half the opening, in (0, 180]), blend (0.15, in [0, 1]: the share of the
 * angle over which the light falls off), soft_shadows (false), shadowFuzzyness (1), samples (8), light_enabled, cast_shadows; with_caustic
 * and with_diffuse are read and dropped.  Accepted only when both `from` and `to` are given (the reference would aim the light from the
 * origin down -z); refused as well: from equal to to, a cone_angle or blend outside its range or not finite, samples below 1 with
 * soft_shadows.  Without soft_shadows a Dirac light, with it a sampled light of `samples` samples that takes both halves of the MIS pair
 * (and is darker for it, as in the reference: SpotLight::intersect almost never answers the BSDF half). */
yafaray_light_t *yafaray_createLight(yafaray_interface_t *yi, const char *name);            /* :92 */
yafaray_texture_t *yafaray_createTexture(yafaray_interface_t *yi, const char *name);        /* :93: type "image" (TGA, HDR and PNG files; none /
                                                                                               bilinear interpolation); procedural types are refused */
yafaray_material_t *yafaray_createMaterial(yafaray_interface_t *yi, const char *name);      /* :94 */
yafaray_camera_t *yafaray_createCamera(yafaray_interface_t *yi, const char *name);          /* :95 */
yafaray_background_t *yafaray_createBackground(yafaray_interface_t *yi, const char *name);  /* :96: types "constant", "textureback",
                                                                                               "gradientback" (with horizon_color and zenith_color)
                                                                                               and "sunsky" (with from; add_sun is refused), each
                                                                                               with or without its background light; "darksky" and
                                                                                               the bare sky calls are refused */
yafaray_integrator_t *yafaray_createIntegrator(yafaray_interface_t *yi, const char *name);  /* :97 */
void yafaray_clearAll(yafaray_interface_t *yi);                                             /* :101 */
/* not in the reference's Interface: an image texture over RGBA float texels the caller holds (row major, as the reference's
 * ImageHandler::getPixel(x, y) would return them), configured by the current ParamMap like createTexture; and the decoded image
 * behind a texture (the file decoders' test hook) */
yafaray_texture_t *yafaray_createTextureFromMemory(yafaray_interface_t *yi, const char *name, int width, int height, const float *rgba);
yafaray_bool_t yafaray_getTextureImage(yafaray_interface_t *yi, const char *name, int *width, int *height, float *rgba, int n_floats);
/* refused with a diagnostic (NULL / 0 and yafaray_getLastError): */
unsigned int yafaray_createObject(yafaray_interface_t *yi, const char *name);               /* :100 */
void *yafaray_createVolumeRegion(yafaray_interface_t *yi, const char *name);                /* :98 */
/* ---- image file output: createImageHandler + ImageOutput + render, the sequence an exporter writes for a file render ----
 * createImageHandler (:99; TgaHandler::factory, imagehandler_tga.cc:525-556, and its siblings) reads from the current ParamMap: type "tga",
 * "hdr" / "pic" or "png"; width and height; alpha_channel (false); for_output (true).  The handler is the buffer an image output fills
 * and the encoder that saves it: 8-bit RGB[A] for tga and png, RGBE for hdr (which has no alpha).  Refused, each with its cause: no type
 * (so the bare call stays refused); jpg / jpeg / tif / tiff / exr (no encoder in this build); any other type; width or height below 1;
 * denoiseEnabled (OpenCV); img_grayscale; with add_to_table, a name that is taken.  for_output = false is accepted and yields a handler
 * without a buffer, which createImageOutput refuses.  No badge is drawn and the height is not extended for one.  The handler is owned by
 * the interface until clearAll; an image output made from it keeps it alive. */
typedef struct yafaray_image_handler yafaray_image_handler_t;
typedef struct yafaray_image_output yafaray_image_output_t;
yafaray_image_handler_t *yafaray_createImageHandler(yafaray_interface_t *yi, const char *name, yafaray_bool_t add_to_table); /* :99 */
/* ImageOutput (common/output_image.cc): the render window goes into the handler's image at (border_x, border_y) and flush writes ONE file
 * under `path` as it is given, as ImageOutput::flush:106-114 does for the combined pass with one view; no log, HTML or statistics file.
 * Owned by the caller; destroy it after the interface's last render with it.  NULL for a null argument, a handler made with for_output =
 * false or a negative border.  yafaray_imageOutputLastError: why the output's last flush failed ("" when it did not). */
yafaray_image_output_t *yafaray_createImageOutput(yafaray_interface_t *yi, yafaray_image_handler_t *handler, const char *path, int border_x, int border_y);
void yafaray_destroyImageOutput(yafaray_image_output_t *image_output);
const char *yafaray_imageOutputLastError(const yafaray_image_output_t *image_output);
/* The image output as a ColorOutput: `user` is the image output, putPixel and flush are the library's own functions, the table lives as long
 * as the image output.  yafaray_render, yafaray_setOutput2 and yafaray_getRenderedImage recognise the table by its putPixel pointer and
 * then do not call it per pixel: one kernel converts the device film into the handler's packed pixels (include/yafgpu.h,
 * yafgpu_scene_film_to_image), one download brings them into the handler's buffer, and flush writes the file.  As output 2 it gets
 * color_space2 / gamma2.  A caller that drives the table itself, pixel by pixel, gets the same file: putPixel stores at (x + border_x,
 * y + border_y), dropping what falls outside the image, and flush packs on the host and saves.
 * yafaray_render refuses, before anything is launched: a render window plus border that does not fit the handler's size (both are named),
 * and images_autosave_interval_type other than "none".  A file that cannot be written fails the render with the path and the cause. */
const yafaray_output_t *yafaray_imageOutputCallbacks(yafaray_image_output_t *image_output);
/* Two functions that need no interface (the cause of a failure: yafaray_filmLastError, per thread).
 * filmToImage: a film [h][w][5] as yafaray_getFilm / yafaray_readFilmFile return it is uploaded, converted by the output stage and
 * downloaded into `out`: w * h pixels of `format` (the YAFGPU_IMAGE_* of include/yafgpu.h: 0 four floats, 1 RGBA8, 2 RGBE).  color_space is
 * "sRGB" | "XYZ" | "LinearRGB" | "Raw_Manual_Gamma".  A merged film file becomes a picture without a render.  Needs a GPU.
 * writeImageFile: host only.  file_type "tga" | "png" (packed_pixels: w * h RGBA8; without alpha the fourth byte is not written) or
 * "hdr" | "pic" (w * h RGBE; alpha is ignored). */
yafaray_bool_t yafaray_filmToImage(const float *film_hw5, int w, int h, const char *color_space, float gamma, yafaray_bool_t alpha, int format, void *out);
yafaray_bool_t yafaray_writeImageFile(const char *path, const char *file_type, int w, int h, yafaray_bool_t alpha, const void *packed_pixels);
/* the calls exporters make around a render besides render() itself */
yafaray_bool_t yafaray_setLoggingAndBadgeSettings(yafaray_interface_t *yi);                 /* :104: accepted; no badge is drawn, no log file written */
yafaray_bool_t yafaray_setupRenderPasses(yafaray_interface_t *yi);                          /* :105: accepted for the combined pass alone; any other enabled pass is refused */
yafaray_bool_t yafaray_setInteractive(yafaray_interface_t *yi, yafaray_bool_t interactive); /* :106 */
int yafaray_getRenderParameters(yafaray_interface_t *yi, char *buf, int len);               /* :108: the render ParamMap as "name=value" lines; returns the bytes needed */
void yafaray_setConsoleVerbosityLevel(yafaray_interface_t *yi, const char *level);          /* :111 */
void yafaray_setLogVerbosityLevel(yafaray_interface_t *yi, const char *level);              /* :112 */
void yafaray_setParamsBadgePosition(yafaray_interface_t *yi, const char *badge_position);   /* :114 */
yafaray_bool_t yafaray_getDrawParams(yafaray_interface_t *yi);                              /* :115 */
void yafaray_printDebug(yafaray_interface_t *yi, const char *msg);                          /* :120-125 */
void yafaray_printVerbose(yafaray_interface_t *yi, const char *msg);
void yafaray_printInfo(yafaray_interface_t *yi, const char *msg);
void yafaray_printParams(yafaray_interface_t *yi, const char *msg);
void yafaray_printWarning(yafaray_interface_t *yi, const char *msg);
void yafaray_printError(yafaray_interface_t *yi, const char *msg);
void yafaray_setOutput2(yafaray_interface_t *yi, const yafaray_output_t *out_2);            /* :128: second output, in color_space2 / gamma2 */

/* Interface::render, interface.cc:411-418 = RenderEnvironment::setupScene (environment.cc:679-813)
 * + Scene::render (scene.cc:1037-1067).  Blocking.  Reads the render settings from the current
 * ParamMap (camera_name, integrator_name, volintegrator_name, background_name, width, height,
 * xstart, ystart, AA_*, filter_type, AA_pixelwidth, tile_size, tiles_order, threads, adv_*).
 * Returns void in the reference; here 1 on success, 0 on failure (yafaray_getLastError). */
yafaray_bool_t yafaray_render(yafaray_interface_t *yi, const yafaray_output_t *output, const yafaray_progress_t *progress);
void yafaray_abort(yafaray_interface_t *yi);                                                 /* :107 */
yafaray_bool_t yafaray_getRenderedImage(yafaray_interface_t *yi, int num_view, const yafaray_output_t *output); /* :109 */

/* ---- additions for measurement and multi-GPU drivers (no reference counterpart) ---- */
typedef struct yafaray_render_stats
{
	uint64_t rays_closest, rays_shadow, interior_steps, leaves, tri_tests, camera_samples, restarts;
	double tree_build_seconds, upload_seconds, render_seconds; /* render_seconds: device time of the pass */
	uint32_t kd_nodes, kd_leaf_refs, kd_max_depth, n_triangles;
	uint64_t scene_device_bytes;
} yafaray_render_stats_t;
/* The float film of the last render: height*width*5 floats {r,g,b,a,weight} — the payload of the
 * reference's film file (imagefilm.cc:1560-1657), i.e. what its ImageFilm holds before normalisation. */
yafaray_bool_t yafaray_getFilm(yafaray_interface_t *yi, float *film, int width, int height);
yafaray_bool_t yafaray_getRenderStats(yafaray_interface_t *yi, yafaray_render_stats_t *stats);
/* ---- film files: save, merge and resume renders (ImageFilm::imageFilmSave / imageFilmLoad / imageFilmLoadAllInFolder /
 * imageFilmFileBackup, imagefilm.cc:1330-1685) ----
 * The file, little-endian: "YAF_FILMv1" 0x00 | the eleven words below | (n_passes + n_aux) x h x w x { float r, g, b, a, weight }, rows
 * outermost.  What yafaray_getFilm returns is one such pass. */
typedef struct yafaray_film_header
{
	uint32_t computer_node;          /* adv_computer_node */
	uint32_t base_sampling_offset;   /* adv_base_sampling_offset, before the node's 100000 is added (imagefilm.h:124) */
	uint32_t sampling_offset;        /* samples per pixel taken so far: offset + samples of the last pass that ran (integrator_tiled.cc:270) */
	int32_t w, h, cx0, cx1, cy0, cy1;        /* width, height, xstart, xstart + width, ystart, ystart + height */
	int32_t n_passes, n_aux;
} yafaray_film_header_t;
/* Host functions, usable without a GPU (merge tools).  Both return 0 on failure, with the cause in yafaray_filmLastError (per thread).
 * writeFilmFile writes the combined pass alone: n_passes = 1 and n_aux = 0 go into the file whatever hdr says.  The reference always
 * carries one auxiliary pass (the sampling factor, renderpasses.cc:277-279) and insists on its own counts when it loads, so a file
 * written here is not for the reference to load.
 * readFilmFile accepts n_passes >= 1 and n_aux >= 0, the reference's files among them, and reads pass 0 into film_hw5 (n_floats must be
 * h * w * 5); film_hw5 = NULL reads the header alone.  Refused, with hdr and the buffer untouched: a wrong or unterminated magic, a
 * negative count, and a file whose length is not exactly what its header promises — checked in 64 bits before anything is read or
 * allocated (the reference reads on and takes what its variables held, file.cc:183-188).  Neither throws. */
yafaray_bool_t yafaray_writeFilmFile(const char *path, const yafaray_film_header_t *hdr, const float *film_hw5);
yafaray_bool_t yafaray_readFilmFile(const char *path, yafaray_film_header_t *hdr, float *film_hw5, uint64_t n_floats);
const char *yafaray_filmLastError(void);
/* The stand-in for session__.getPathImageOutput(): the image output path without extension, e.g. "out/frame0007"; this interface's
 * film file is "<path> - node NNNN.film", NNNN = adv_computer_node in four digits (imagefilm.cc:1330-1338).  NULL or "" detaches it.
 * What the render parameter film_save_load then does in yafaray_render (and only there: prepareRender / renderPassDevice callers own
 * their memory):
 *   no film path   nothing, whatever the parameters say (the reference with an output that is no image file, imagefilm.cc:900-904)
 *   "save"         an existing film file of this node is renamed to "<file>-previous.bak" before the render; the film is written after
 *                  a render that finished (an aborted or failed one writes nothing)
 *   "load-save"    first every regular file of the path's directory ("." when it has none) with the extension "film" whose base name
 *                  STARTS WITH the path's base name is loaded, in the order of the sorted path strings, and added to a zero film in
 *                  float32 — this node's own earlier file among them, and "frame1" also takes "frame10 - node 0000.film" (the reference's
 *                  rule, imagefilm.cc:1497-1500).  A file with another w, h, cx0, cx1, cy0 or cy1 than the render, or one readFilmFile
 *                  refuses, is skipped whole; the warnings are in yafaray_getLastError after the render.  sampling_offset and
 *                  base_sampling_offset become the maximum of the render's own and every loaded file's.  With at least one film loaded
 *                  the render is resumed (integrator_tiled.cc:196-203): pass 1 is skipped — it still spends its tile seeds — and the
 *                  adaptive passes 1 .. AA_passes - 1 go on from the loaded sampling_offset; AA_passes = 1 only combines the films.
 *                  With none it is an ordinary render.  Then the backup and the final save as for "save".
 *   anything else  "none" (environment.cc:524-526)
 * Refused by yafaray_render with a film path set: film_autosave_interval_type other than "none" (no autosave between passes), and a
 * saving or loading mode with shard_count > 1 (a rank's film is its share of the frame). */
void yafaray_setFilmPath(yafaray_interface_t *yi, const char *path);
const char *yafaray_getFilmPath(const yafaray_interface_t *yi);
/* what the last yafaray_render loaded: the number of film files (0: an ordinary render) and the merged offsets; any pointer may be NULL */
void yafaray_getFilmResume(yafaray_interface_t *yi, int *n_loaded, unsigned int *sampling_offset, unsigned int *base_sampling_offset);
/* pixel-tile sharding: must be set before render; tile t belongs to shard t % count */
void yafaray_setShard(yafaray_interface_t *yi, int shard_index, int shard_count);
/* Multi-pass (adaptive) anti-aliasing on a sharded frame: between passes the noise detection (integrator_tiled.cc:136-258)
 * needs every rank's pixels.  `fn` receives a copy of this rank's splat planes in DEVICE memory and must sum it over all ranks
 * in place (an all-reduce; libyafaray_amd/parallel.py does it with torch.distributed = RCCL) and return 0.  Without it a sharded
 * multi-pass render is refused.  The film a rank returns stays its own share (sum them as for a one-pass render).
 * The same function carries the light counter of the serial replay below across ranks (a small table of per-tile call counts once per
 * pass): with it a sharded render of a scene with several lights makes the single-GPU render's light choices; without it, its own.
 * The exchange is a collective: a rank that fails or is aborted (yafaray_abort) before it leaves the others waiting in theirs, as with
 * any collective — abort a sharded render on EVERY rank (the flag is polled between chunks and passes, before each exchange). */
typedef int (*yafaray_plane_exchange_t)(void *user, float *d_values, uint64_t n_floats);
void yafaray_setPlaneExchange(yafaray_interface_t *yi, yafaray_plane_exchange_t fn, void *user);
/* ---- multi-GPU: one process per GPU, RCCL over xGMI, no Python on the data path (yafaray_reduce.cpp) -------------------------
 * The reference's only multi-machine mechanism sums film files (imagefilm.cc:1467-1557: col += , weight +=); here each rank
 * renders its tile shard into a full-frame [H][W][5] float film and ONE ncclReduce(sum) assembles the frame on `root`.
 * Sequence for N ranks: rank 0 yafaray_commGetUniqueId -> the host hands the 128 bytes to every rank (file,
 * environment, MPI, a socket) -> each rank yafaray_commCreate(id, rank, N, device) -> yafaray_setShard(yi, rank, N) ->
 * yafaray_setComm(yi, comm) -> render into device memory -> yafaray_reduceFilm.  RCCL is loaded at run time; without it these
 * functions fail with a message in yafaray_commLastError (there is no host-staged fallback). */
#define YAFARAY_COMM_ID_BYTES 128
typedef struct yafaray_comm yafaray_comm_t;
yafaray_bool_t yafaray_commGetUniqueId(char id[YAFARAY_COMM_ID_BYTES]);
yafaray_comm_t *yafaray_commCreate(const char id[YAFARAY_COMM_ID_BYTES], int rank, int world, int device);
void yafaray_commDestroy(yafaray_comm_t *comm);
int yafaray_commRank(const yafaray_comm_t *comm);
int yafaray_commWorld(const yafaray_comm_t *comm);
const char *yafaray_commLastError(void);
const char *yafaray_commBackend(void);      /* which librccl was bound ("" when none) */
/* sum of the ranks' device films onto `root`, in place, asynchronously on `stream` (ncclReduce); n_floats = height*width*5 */
yafaray_bool_t yafaray_reduceFilm(yafaray_comm_t *comm, float *d_film, uint64_t n_floats, int root, void *stream);
/* sum over all ranks, in place on every rank (ncclAllReduce) */
yafaray_bool_t yafaray_allReduce(yafaray_comm_t *comm, float *d_values, uint64_t n_floats, void *stream);
/* the communicator as a yafaray_plane_exchange_t (user = the communicator) */
int yafaray_commExchange(void *user, float *d_values, uint64_t n_floats);
/* attach a communicator to an interface: yafaray_setPlaneExchange(yi, yafaray_commExchange, comm); NULL detaches */
void yafaray_setComm(yafaray_interface_t *yi, yafaray_comm_t *comm);

/* Exact replay of the reference's serial render state (on by default): the per-tile Random that Russian roulette draws from
 * (integrator_tiled.cc:319, seeded from libc rand() as the last Material / ObjectGeometric constructor left it;
 * integrator_path_tracer.cc:282-288) and the estimateOneDirectLight counter (integrator_montecarlo.cc:62-76), both as a
 * single-threaded render with tiles_order = linear consumes them.  Costs a record pass of closest-hit rays per chunk when a
 * render consumes either (RR active, or more than one light).  Off: per-sample streams — the same estimator, other pixels. */
void yafaray_setSerialReplay(yafaray_interface_t *yi, yafaray_bool_t on);
/* srand() seed and values consumed since, of the libc stream the next render's tile seeds continue (-1: nothing created yet) */
void yafaray_getRandState(yafaray_interface_t *yi, int *srand_seed, int *skip);
/* An embedder that calls libc srand(seed) itself (and consumes `skip` values) between scene construction and render says so
 * here — the reference would simply continue from that state at integrator_tiled.cc:319.  Holds until the next material or
 * object is created (their constructors call srand again).  seed < 0: back to the constructors' state. */
void yafaray_setRandState(yafaray_interface_t *yi, int srand_seed, int skip);
/* Two-step render for drivers that own device memory and streams (bench.py, RCCL reduce):
 * prepare = setupScene + Scene::update (tree build, upload); renderPass launches one pass
 * asynchronously on `stream` into caller-owned device memory d_planes (yafgpu_planes_bytes). */
yafaray_bool_t yafaray_prepareRender(yafaray_interface_t *yi);
yafaray_bool_t yafaray_renderPassDevice(yafaray_interface_t *yi, float *d_planes, void *d_counters, void *stream);
yafaray_bool_t yafaray_getRenderSize(yafaray_interface_t *yi, int *width, int *height);
/* Scene::intersect / Scene::isShadowed (scene.cc:896-994) on host ray batches, after prepareRender:
 * rays = n*8 floats {from.xyz, dir.xyz, tmin, tmax (<0 = infinite)}; tri = -1 on a miss */
yafaray_bool_t yafaray_intersectRays(yafaray_interface_t *yi, int n, const float *rays, int *tri, float *t, float *bary);
yafaray_bool_t yafaray_shadowRays(yafaray_interface_t *yi, int n, const float *rays, int *shadowed);
/* per-kernel device timing of the next renderPassDevice (yafgpu_set_profiling / yafgpu_get_profile):
 * ms[4]/launches[4] = closest-hit traversal, any-hit traversal, shading, other */
yafaray_bool_t yafaray_setProfiling(yafaray_interface_t *yi, yafaray_bool_t enable);
yafaray_bool_t yafaray_getKernelProfile(yafaray_interface_t *yi, double ms[4], uint64_t launches[4]);
/* consecutive renderPassDevice calls of independent passes on two internal streams (yafgpu_scene_set_pass_pipelining, include/yafgpu.h):
 * -1 by size (default), 0 off, 1 on.  What the caller sees — planes, counters — is written on the caller's stream, in call order, either way. */
yafaray_bool_t yafaray_setPassPipelining(yafaray_interface_t *yi, int mode);
/* device-side component probe (yafgpu_probe) against the prepared scene's materials/lights/camera */
yafaray_bool_t yafaray_probe(yafaray_interface_t *yi, int op, int n, const float *in, int n_in, float *out, int n_out);

/* XML scene loader: src/loader_xml/loader_xml.cc + src/common/import_xml.cc drive the same calls
 * from a scene file.  Parses `path` and leaves the interface ready for yafaray_render. */
yafaray_bool_t yafaray_loadXml(yafaray_interface_t *yi, const char *path);

#ifdef __cplusplus
}
#endif
#endif
