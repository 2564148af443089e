#!/usr/bin/env python3
"""tests/golden/reference_facts.json -- what the reference's own text says, recorded as data (numbers, names, yes / no answers).

tests/test_reference_constants.py, tests/test_reference_structure.py and tests/test_functor_ref.py hold the oracle and the HIP path to the
reference's text.  The reference is not part of this repository, so the readings are made here, once, from a
checkout of it, and the tests read the recorded answers: the constants of kitti.h, the start-up transform of main.cpp, the LRU capacity
of lru.h, the loss / threshold / weight of every residual block and the solver options of velo.h, one yes / no per line the oracle
restates "as written", and the digests of the functor vectors make_functor_ref.py computes from costfunctions.h.  Nothing of the
reference's text is stored.

    python tests/golden/make_reference_facts.py REFERENCE_DIR            # writes tests/golden/reference_facts.json
    python tests/golden/make_reference_facts.py REFERENCE_DIR --check    # exit 1 if the committed file differs from a fresh reading"""
import hashlib
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "reference_facts.json")
FRAME_FUNCTORS = ("cost3D3D", "cost3D2D", "cost2D3D", "cost2D2D", "cost3DPD")


def array_digest(a):
    a = np.ascontiguousarray(a)
    return hashlib.sha256(repr((a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


def _read(ref, name):
    return open(os.path.join(ref, name)).read()


def kitti_constants(text):
    """`name = value` pairs of the two constant lists at the top of kitti.h (const int ...; const double ...;)"""
    out = {}
    for block in re.findall(r"const\s+(?:int|double)\s+(.*?);", text, flags=re.S):
        block = re.sub(r"//[^\n]*", "", block)
        for name, value in re.findall(r"(\w+)\s*=\s*([-+0-9.eE]+)", block):
            out[name] = float(value)
    return out


def loss_sites(text):
    """{functor: [dim, loss class, threshold name, weight name or None]} from every AddResidualBlock of frameToFrame"""
    body = text[text.index("Eigen::Matrix4d frameToFrame("):text.rindex("void residualStats(")]
    out = {}
    for m in re.finditer(r"AutoDiffCostFunction<\s*(cost\w+)\s*,\s*(\d)\s*,\s*6\s*>", body):
        tail = body[m.end():m.end() + 1200]
        tail = tail[tail.index("AddResidualBlock("):]
        tail = tail[:tail.index("transform)")]
        scaled = re.search(r"ScaledLoss\(\s*new\s+ceres::(\w+Loss)\((\w+)\)\s*,\s*(\w+)", tail)
        plain = re.search(r"new\s+ceres::(\w+Loss)\((\w+)\)", tail)
        if not (scaled or plain):
            raise ValueError(f"no loss found for {m.group(1)}")
        out[m.group(1)] = [int(m.group(2))] + ([scaled.group(1), scaled.group(2), scaled.group(3)] if scaled else [plain.group(1), plain.group(2), None])
    return out


def solver_options(text):
    body = text[text.index("Eigen::Matrix4d frameToFrame("):]
    body = body[:body.index("ceres::Solve(options")]
    return dict(re.findall(r"^\s*options\.(\w+)\s*=\s*([^;]+);", body, flags=re.M))


def as_written(ref):
    """one yes / no per restated line (the file and line numbers are the reference's)"""
    velo = _read(ref, "velo.h")
    v = re.sub(r"\s+", "", velo)
    u_raw = _read(ref, "utility.h")
    u = re.sub(r"\s+", "", u_raw)
    k = re.sub(r"\s+", "", _read(ref, "kitti.h"))
    f = {}
    # velo.h:829 -- the correspondence gate is correspondence_thresh_icp / iter^4 on the squared distance
    f["icp_gate_divides_by_iter_four_times"] = bool(re.search(r"correspondence_thresh_icp\s*/\s*iter\s*/\s*iter\s*/\s*iter\s*/\s*iter", velo))
    # velo.h:836,843,859 / 806-807 / 828-829 / 873
    f["ring_scan_strict_less_then_else_if"] = bool(re.search(r"if\s*\(\s*d\s*<\s*np_dist_i\s*\)", velo) and re.search(r"else\s+if\s*\(\s*d\s*<\s*np_dist_j\s*\)", velo))
    f["plus_one_neighbour_only_when_strictly_closer"] = bool(re.search(r"if\s*\(\s*util::norm2\(np_k_1\)\s*<\s*util::norm2\(np_k_2\)\s*\)", velo))
    f["ring_loop_bound_times_enable_icp"] = bool(re.search(r"sm\s*<\s*scans_M\.size\(\)\s*\*\s*enable_icp", velo))
    f["point_loop_strides_by_icp_skip_from_zero"] = bool(re.search(r"smi\s*=\s*0\s*;\s*smi\s*<\s*scans_M\[sm\]->size\(\)\s*;\s*smi\s*\+=\s*icp_skip", velo))
    f["ring_counts_when_search_found_something"] = bool(re.search(r"nearestKSearch\(\s*pointM\s*,\s*1\s*,\s*id\s*,\s*dist2\s*\)\s*<=\s*0", velo))
    f["degenerate_planes_skipped_by_icp_norm_condition"] = bool(re.search(r"icp_norm_condition", velo))
    # utility.h:35-39,51-53,97-103 and the pose conversions
    m = re.search(r"subtract_assign\(pcl::PointXYZ\s*&a,\s*const\s+pcl::PointXYZ\s*&b\)\s*\{(.*?)\}", u_raw, flags=re.S)
    f["subtract_assign_componentwise_float_in_place"] = bool(m and re.sub(r"\s", "", m.group(1)) == "a.x-=b.x;a.y-=b.y;a.z-=b.z;")
    m = re.search(r"static\s+inline\s+double\s+norm2\(const\s+pcl::PointXYZ\s*&p\)\s*\{(.*?)\}", u_raw, flags=re.S)
    f["norm2_float_expression_returned_as_double"] = bool(m and re.sub(r"\s", "", m.group(1)) == "returnp.x*p.x+p.y*p.y+p.z*p.z;")
    m = re.search(r"transform_point\(pcl::PointXYZ\s*&p,\s*const\s+double\s+transform\[6\]\)\s*\{(.*?)\n    \}", u_raw, flags=re.S)
    f["transform_point_rotates_and_adds_in_double_stores_float"] = bool(m and re.sub(r"\s", "", m.group(1)) ==
                                                                        "doublex[3]={p.x,p.y,p.z},y[3]={0,0,0};ceres::AngleAxisRotatePoint(transform,x,y);p.x=y[0]+transform[3];p.y=y[1]+transform[4];p.z=y[2]+transform[5];")
    f["pose_conversions_column_major"] = bool(re.search(r"T\(i,\s*j\)\s*=\s*R\[j\*3\s*\+\s*i\]", u_raw) and re.search(r"R\[j\*3\s*\+\s*i\]\s*=\s*T\(i,\s*j\)", u_raw))
    # velo.h:674-682,709,739-742,772-775 -- the visual gates
    for t, n in (("3D3D", 3), ("3D2D", 2)):
        sq = "+".join(f"residual_test[{i}]*residual_test[{i}]" for i in range(n))
        f[f"visual_gate_{t}_squared_norm_left_to_right_from_second_iteration"] = f"if(iter>1&&{sq}>loss_thresh_{t}*outlier_reject/iter*loss_thresh_{t}*outlier_reject/iter)" in v
    f["visual_gate_3D2D_threshold_shared_by_two_blocks"] = v.count("*loss_thresh_3D2D*outlier_reject/iter)continue;") == 2
    f["visual_gate_2D2D_absolute_value"] = "if(iter>1&&abs(residual_test[0])>loss_thresh_2D2D*outlier_reject/iter)continue;" in v
    # kitti.h:164-183 -- the ring segmenter
    f["segmenter_new_ring_where_x_positive_and_y_flips"] = "floatprev_y=0;" in k and "if(i>0&&p.x>0&&(p.y>0)!=(prev_y>0)){scan_id++;}" in k
    f["segmenter_ring_reorder_and_velo_to_cam"] = "cloud_tmp->at(scan_ids[s][_i-1-(i+_i/2)%_i])" in k and "pcl::transformPointCloud(*point_cloud,*cloud_tmp,velo_to_cam);" in k
    # utility.h:7-29, velo.h:345-366,397-422,1078-1122 -- the widened rows
    f["linterpolate_in_float"] = (u.count("floata=(mid-start)/(end-start);floatb=1-a;") == 2 and "floatx=p1.x*b+p2.x*a;floaty=p1.y*b+p2.y*a;floatz=p1.z*b+p2.z*a;" in u
                                  and "returnp1*b+p2*a;" in u)
    f["projection_and_window_test"] = ("pcl::PointXYZpp(p.x+t(0),p.y+t(1),p.z+t(2));cv::Point2fc(pp.x/pp.z,pp.y/pp.z);" in v
                                       and "if(pp.z>0&&c.x>=min_x[cam]&&c.x<max_x[cam]&&c.y>=min_y[cam]&&c.y<max_y[cam])" in v)
    f["occlusion_stack_rules"] = ("while(projection[s].size()>0&&c.x<projection[s].back().x&&pp.z<projected_points.back().z)" in v
                                  and "if(projection[s].size()>0&&c.x<projection[s].back().x&&pp.z>projected_points.back().z){bad++;continue;}" in v)
    f["depth_association_bisection_and_acceptance"] = (
        "if(projection[s].size()<=1){last_interp=-1;continue;}" in v
        and "intlo=0,hi=projection[s].size()-2,mid=0;while(lo<=hi){mid=(lo+hi)/2;if(projection[s][mid].x>kp.x){hi=mid-1;}elseif(projection[s][mid+1].x<=kp.x){lo=mid+1;}else{found=true;" in v
        and ("if(last_interp!=-1&&(projection[s][mid].y>kp.y)!=(projection[s-1][last_interp].y>kp.y)&&abs(projection[s][mid].x-projection[s][mid+1].x)<depth_assoc_thresh"
             "&&abs(projection[s-1][last_interp].x-projection[s-1][last_interp+1].x)<depth_assoc_thresh)") in v)
    tri = v[v.index("triangulatePoint("):]
    f["triangulation_losses"] = "newceres::TrivialLoss," in tri and "newceres::ScaledLoss(newceres::CauchyLoss(loss_thresh_3D2D),weight_3D2D,ceres::TAKE_OWNERSHIP)" in tri
    # velo.h:921-1025 -- residualStats
    st = v[v.rindex("voidresidualStats("):v.index("Eigen::Vector3dtriangulatePoint(") if "Eigen::Vector3dtriangulatePoint(" in v else len(v)]
    f["residual_stats_without_loss"] = "evaluate_options.apply_loss_function=false;" in st
    f["residual_stats_block_norms"] = ("residuals_3D3D.push_back(sqrt(residuals[ri]*residuals[ri]+residuals[ri+1]*residuals[ri+1]+residuals[ri+2]*residuals[ri+2]));ri+=3;" in st
                                       and st.count("sqrt(residuals[ri]*residuals[ri]+residuals[ri+1]*residuals[ri+1]));ri+=2;") == 2
                                       and "residuals_2D2D.push_back(abs(residuals[ri]));ri++;" in st
                                       and "for(;ri<residuals.size();ri++){residuals_3DPD.push_back(abs(residuals[ri]));}" in st)
    f["residual_stats_sum_before_sort"] = st.index("for(autor:residuals_3DPD){sum_3DPD+=r;}") < st.index("std::sort(residuals_3D3D.begin(),residuals_3D3D.end());")
    f["residual_stats_median_and_mean_per_type"] = all(f"residuals_{t}[residuals_{t}.size()/2]" in st and f"sum_{t}/residuals_{t}.size()" in st
                                                       for t in ("3D3D", "3D2D", "2D3D", "2D2D", "3DPD"))
    return f


def read_facts(ref):
    main = _read(ref, "main.cpp")
    m = re.search(r"double\s+transform\[6\]\s*=\s*\{([^}]*)\}", main)
    lru = re.search(r"class\s+ScansLRU\s*\{.*?const\s+int\s+size\s*=\s*(\d+)", _read(ref, "lru.h"), flags=re.S)
    velo = _read(ref, "velo.h")
    sys.path.insert(0, HERE)
    import make_functor_ref as M
    header = os.path.join(ref, "costfunctions.h")
    fresh = M.generate(header)
    parsed = M.parse_functors(open(header).read())
    return {
        "kitti_constants": kitti_constants(_read(ref, "kitti.h")),
        "startup_transform": [float(x) for x in m.group(1).split(",")],
        "scans_lru_size": int(lru.group(1)),
        "loss_sites": loss_sites(velo),
        "solver_options": solver_options(velo),
        "as_written": as_written(ref),
        "functor_parameter_counts": {n: len(parsed[n][0]) for n in (*FRAME_FUNCTORS, "triangulation2D", "triangulation3D")},
        "functor_vector_digests": {k: array_digest(v) for k, v in sorted(fresh.items())},
    }


if __name__ == "__main__":
    if len(sys.argv) < 2 or not os.path.isdir(sys.argv[1]):
        sys.exit(__doc__)
    facts = read_facts(sys.argv[1])
    text = json.dumps(facts, indent=1, sort_keys=True) + "\n"
    if "--check" in sys.argv[2:]:
        same = os.path.exists(OUT) and open(OUT).read() == text
        print("reference_facts.json is " + ("what the reference says" if same else "NOT what the reference says"))
        sys.exit(0 if same else 1)
    open(OUT, "w").write(text)
    print(f"wrote {OUT}")
