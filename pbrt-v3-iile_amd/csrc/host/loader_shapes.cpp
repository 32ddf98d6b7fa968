// loader_shapes.cpp — the `Shape` directive: spheres, disks and cylinders, and the three sources of triangle meshes; each
// primitive gets the open area light attached (pbrt_loader.h).
#include "pbrt_loader.h"

namespace iile {

bool Loader::make_shape(const std::string &name, const ParamSet &ps) {
    // pbrtShape under an animated CTM (api.cpp:1406-1447) makes a TransformedPrimitive over a BVH of the shape's own: a moving
    // instance, which this path does not have. Refused by name: the camera's motion alone is rendered.
    if (ctms_.animated())
        return fail(std::string("Shape \"") + name + "\"" + (gs_.has_area_light ? " (and the AreaLightSource on it)" : "") +
                    " under an animated transform (ActiveTransform) is not supported: camera motion only, moving shapes are not rendered");
    HostPrim pr;  // what every primitive of this shape starts from
    pr.flags = (gs_.reverse_orientation ^ ctm().swaps_handedness()) ? IILE_PRIM_FLIP : 0;
    pr.material = current_material();
    if (pr.material < 0) return false;
    if (name == "sphere") {
        sphere_shape(ps, &pr);
        return true;
    }
    if (name == "disk" || name == "cylinder") return quadric_shape(name, ps, &pr);
    if (name != "plymesh" && name != "trianglemesh" && name != "loopsubdiv")  // cone, paraboloid, hyperboloid, curve, heightfield, nurbs
        return fail("Shape \"" + name + "\" is not supported (sphere, disk, cylinder, trianglemesh, plymesh, loopsubdiv)");
    return mesh_shape(name, ps, pr);
}

// pbrtShape (api.cpp:1403-1419): the primitive joins the scene, with a DiffuseAreaLight of its own (`light_type` says on what
// kind of shape) if an AreaLightSource is open
void Loader::add_primitive(int light_type, HostPrim *pr) {
    if (gs_.has_area_light) {
        iile_light lt = diffuse_area_light();
        lt.type = light_type;
        if (light_type == IILE_LIGHT_DIFFUSE_AREA)
            lt.sphere = pr->shape;
        else
            lt.prim = -1;  // set once the primitives are in BVH order (finalize_scene)
        scene_->lights.push_back(lt);
        pr->light = int(scene_->lights.size()) - 1;
    }
    scene_->prims.push_back(*pr);
}

void Loader::sphere_shape(const ParamSet &ps, HostPrim *pr) {  // shapes/sphere.cpp:318-327, sphere.h:50-60
    const Xform &o2w = ctm();
    float radius = ps.one_float("radius", 1.f);
    float zmin = ps.one_float("zmin", -radius);
    float zmax = ps.one_float("zmax", radius);
    float phimax = ps.one_float("phimax", 360.f);
    iile_sphere sp;
    std::memset(&sp, 0, sizeof(sp));
    std::memcpy(sp.o2w, o2w.m.m, sizeof(sp.o2w));
    std::memcpy(sp.o2w_inv, o2w.inv.m, sizeof(sp.o2w_inv));
    sp.radius = radius;
    sp.zmin = clampT(std::min(zmin, zmax), -radius, radius);
    sp.zmax = clampT(std::max(zmin, zmax), -radius, radius);
    sp.theta_min = std::acos(clampT(std::min(zmin, zmax) / radius, -1.f, 1.f));
    sp.theta_max = std::acos(clampT(std::max(zmin, zmax) / radius, -1.f, 1.f));
    sp.phi_max = radians(clampT(phimax, 0.f, 360.f));
    sp.reverse_orientation = gs_.reverse_orientation;
    sp.swaps_handedness = o2w.swaps_handedness();
    scene_->spheres.push_back(sp);
    pr->flags |= IILE_PRIM_SPHERE;
    pr->shape = int(scene_->spheres.size()) - 1;
    // Shape::WorldBound = ObjectToWorld(ObjectBound()), shape.cpp:54, sphere.cpp:43-46
    pr->world_bound = o2w.bounds(Bounds3(V3(-radius, -radius, sp.zmin), V3(radius, radius, sp.zmax)));
    add_primitive(IILE_LIGHT_DIFFUSE_AREA, pr);
}

bool Loader::quadric_shape(const std::string &name, const ParamSet &ps, HostPrim *pr) {
    const Xform &o2w = ctm();
    iile_quadric q;
    std::memset(&q, 0, sizeof(q));
    std::memcpy(q.o2w, o2w.m.m, sizeof(q.o2w));
    std::memcpy(q.o2w_inv, o2w.inv.m, sizeof(q.o2w_inv));
    q.reverse_orientation = gs_.reverse_orientation;
    q.swaps_handedness = o2w.swaps_handedness();
    Bounds3 ob;
    if (name == "disk") {  // CreateDiskShape, shapes/disk.cpp:140-150, and the constructor, disk.h:50-57
        q.kind = IILE_QUADRIC_DISK;
        q.height = ps.one_float("height", 0.f);
        q.radius = ps.one_float("radius", 1.f);
        q.inner_radius = ps.one_float("innerradius", 0.f);
        q.phi_max = radians(clampT(ps.one_float("phimax", 360.f), 0.f, 360.f));
        ob = Bounds3(V3(-q.radius, -q.radius, q.height), V3(q.radius, q.radius, q.height));  // disk.cpp:43-46
    } else {  // CreateCylinderShape, shapes/cylinder.cpp:223-233, and the constructor, cylinder.h:50-57
        q.kind = IILE_QUADRIC_CYLINDER;
        q.radius = ps.one_float("radius", 1.f);
        const float zmin = ps.one_float("zmin", -1.f), zmax = ps.one_float("zmax", 1.f);
        q.zmin = std::min(zmin, zmax);
        q.zmax = std::max(zmin, zmax);
        q.phi_max = radians(clampT(ps.one_float("phimax", 360.f), 0.f, 360.f));
        ob = Bounds3(V3(-q.radius, -q.radius, q.zmin), V3(q.radius, q.radius, q.zmax));  // cylinder.cpp:43-46
    }
    scene_->quadrics.push_back(q);
    pr->flags |= IILE_PRIM_QUADRIC;
    pr->shape = int(scene_->quadrics.size()) - 1;
    pr->world_bound = o2w.bounds(ob);  // Shape::WorldBound, shape.cpp:54
    add_primitive(IILE_LIGHT_AREA_QUADRIC, pr);
    return true;
}

// the vertices of a plymesh (shapes/plymesh.cpp:149-300), a trianglemesh (shapes/triangle.cpp:616-714) or a loopsubdiv
// (shapes/loopsubdiv.cpp:402-424), in object space
bool Loader::mesh_source(const std::string &name, const ParamSet &ps, std::vector<int> *indices, std::vector<V3> *P, std::vector<V3> *N,
                         std::vector<float> *uv) {
    if (name == "plymesh") {
        const std::string fn = ps.one_string("filename", "");
        if (fn.empty()) return fail("plymesh: \"filename\" is required");
        std::string perr;
        return load_ply(in_search_dir(fn), P, N, uv, indices, &perr) || fail(perr);
    }
    const Param *pi = ps.find("indices");
    const Param *pp = ps.find("P");
    if (!pi || !pp) return fail("Shape " + name + ": \"indices\" and \"P\" are required");
    for (double v : pi->nums) indices->push_back(int(v));
    for (size_t i = 0; i + 2 < pp->nums.size(); i += 3)
        P->push_back(V3(float(pp->nums[i]), float(pp->nums[i + 1]), float(pp->nums[i + 2])));
    if (name == "trianglemesh") {
        const Param *pu = ps.find("uv");
        if (!pu) pu = ps.find("st");
        if (pu) {
            for (double v : pu->nums) uv->push_back(float(v));
            if (uv->size() / 2 < P->size()) uv->clear();
        }
        const Param *pn = ps.find("N");
        if (pn && pn->nums.size() == 3 * P->size())
            for (size_t i = 0; i + 2 < pn->nums.size(); i += 3)
                N->push_back(V3(float(pn->nums[i]), float(pn->nums[i + 1]), float(pn->nums[i + 2])));
        if (ps.find("S")) return fail("trianglemesh \"S\" tangents are not supported");
    } else {  // loopsubdiv
        int levels = ps.one_int("levels", ps.one_int("nlevels", 3));
        std::vector<int> oi;
        std::vector<V3> oP, oN;
        loop_subdivide(levels, *indices, *P, &oi, &oP, &oN);
        indices->swap(oi);
        P->swap(oP);
        N->swap(oN);
    }
    return true;
}

// "alpha" / "shadowalpha": a float texture by name, or a float that masks everything when it is 0
// (CreateTriangleMeshShape, triangle.cpp:689-710; CreatePLYMesh, plymesh.cpp:259-285)
bool Loader::alpha_masks(const ParamSet &ps, int alpha_mask[2]) {
    const char *pnames[2] = {"alpha", "shadowalpha"};
    for (int k = 0; k < 2; ++k) {
        const Param *pa = ps.find(pnames[k]);
        if (!pa) continue;
        if (pa->type == "texture") {
            if (pa->strs.size() != 1) return fail(std::string("bad texture reference for \"") + pnames[k] + "\"");
            const ConstTexture *t = named_texture(pa);
            if (!t || !t->is_float)
                return fail("Couldn't find float texture \"" + pa->strs[0] + "\" for \"" + pnames[k] + "\" parameter");
            if (t->image >= 0 && scene_->textures[size_t(t->image)].t.kind != IILE_TEX_IMAGE)
                return fail("procedural texture \"" + pa->strs[0] + "\" as \"" + pnames[k] + "\" is not supported (image textures only)");
            if (t->image >= 0)
                alpha_mask[k] = t->image;
            else if (t->v[0] == 0.f)
                alpha_mask[k] = IILE_ALPHA_ZERO;
        } else if (pa->type == "float" && pa->nums.size() == 1 && float(pa->nums[0]) == 0.f) {
            alpha_mask[k] = IILE_ALPHA_ZERO;
        }
    }
    return true;
}

// one primitive per triangle, each a copy of `proto` with its vertices in world space
bool Loader::mesh_shape(const std::string &name, const ParamSet &ps, const HostPrim &proto) {
    HostScene &s = *scene_;
    const Xform o2w = ctm();
    std::vector<int> indices;
    std::vector<V3> P, N;
    std::vector<float> uv;
    if (!mesh_source(name, ps, &indices, &P, &N, &uv)) return false;
    int alpha_mask[2] = {IILE_ALPHA_NONE, IILE_ALPHA_NONE};
    if (name != "loopsubdiv" && !alpha_masks(ps, alpha_mask)) return false;
    for (int idx : indices)
        if (idx < 0 || idx >= int(P.size())) return fail("trianglemesh has out-of-bounds vertex index");
    // TriangleMesh ctor, shapes/triangle.cpp:54-93: vertices and normals to world space
    std::vector<V3> Pw(P.size()), Nw(N.size());
    for (size_t i = 0; i < P.size(); ++i) Pw[i] = o2w.point(P[i]);
    for (size_t i = 0; i < N.size(); ++i) Nw[i] = o2w.normal(N[i]);
    int mesh_id = s.n_meshes++;
    size_t ntris = indices.size() / 3;
    s.prims.reserve(s.prims.size() + ntris);
    for (size_t t = 0; t < ntris; ++t) {
        HostPrim pr = proto;
        pr.flags |= (N.empty() ? 0 : IILE_PRIM_HAS_NORMALS) | (uv.empty() ? 0 : IILE_PRIM_HAS_UV) |
                    ((alpha_mask[0] != IILE_ALPHA_NONE || alpha_mask[1] != IILE_ALPHA_NONE) ? IILE_PRIM_HAS_ALPHA : 0);
        pr.alpha = alpha_mask[0];
        pr.shadow_alpha = alpha_mask[1];
        pr.shape = mesh_id;
        for (int k = 0; k < 3; ++k) {
            int vi = indices[3 * t + k];
            pr.p[k] = Pw[vi];
            if (!N.empty()) pr.n[k] = Nw[vi];
            if (!uv.empty()) {
                pr.uv[2 * k] = uv[2 * vi];
                pr.uv[2 * k + 1] = uv[2 * vi + 1];
            }
        }
        // Triangle::WorldBound, shapes/triangle.cpp:180-186
        pr.world_bound = bunion(Bounds3(pr.p[0], pr.p[1]), pr.p[2]);
        add_primitive(IILE_LIGHT_AREA_TRIANGLE, &pr);  // one DiffuseAreaLight per shape, i.e. per triangle
    }
    return true;
}

}  // namespace iile
