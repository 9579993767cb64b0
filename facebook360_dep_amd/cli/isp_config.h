// isp.json -> derp_isp_config: the "CameraIsp" object as CameraIsp::CameraIsp reads it (source/isp/CameraIsp.h:521-565).
// Missing keys keep the defaults of derp_isp_config_default; a missing "CameraIsp" object means all defaults. A file
// that is no JSON, or a key of the wrong kind, ends the process like any other bad input: a fatal line, exit status 1.
#pragma once
#include "cli_common.h"

namespace cli {

inline double isp_number(const Json& j, const std::string& key) {
  if (j.kind != Json::Num) {
    LOG_FATAL("isp JSON: '" + key + "' must be a number");
  }
  return j.num;
}
// getPoint (:418-441): null leaves the default; otherwise x, y, z from elements 0..2
inline void isp_point(const Json& obj, const std::string& key, float out[3]) {
  const Json* j = obj.find(key);
  if (!j || j->kind == Json::Null) {
    return;
  }
  if (j->kind != Json::Arr || j->arr.size() < 3) {
    LOG_FATAL("isp JSON: '" + key + "' must be an array of three numbers");
  }
  for (int c = 0; c < 3; ++c) {
    out[c] = (float)isp_number(j->arr[c], key);
  }
}
// getCoordList (:443-454); returns the number of points, -1 when the key is absent
inline int isp_points(const Json& obj, const std::string& key, float (*out)[3], int cap) {
  const Json* j = obj.find(key);
  if (!j || j->kind == Json::Null) {
    return -1;
  }
  if (j->kind != Json::Arr) {
    LOG_FATAL("isp JSON: '" + key + "' must be an array of points");
  }
  if (out && (int)j->arr.size() > cap) {
    LOG_FATAL(fmt("isp JSON: '%s' holds %zu points, at most %d are supported", key.c_str(), j->arr.size(), cap));
  }
  for (size_t n = 0; n < j->arr.size(); ++n) {
    if (j->arr[n].kind != Json::Arr || j->arr[n].arr.size() < 3) {
      LOG_FATAL("isp JSON: '" + key + "' must be an array of points");
    }
    for (int c = 0; c < 3; ++c) {
      const float v = (float)isp_number(j->arr[n].arr[c], key);
      if (out) {
        out[n][c] = v;
      }
    }
  }
  return (int)j->arr.size();
}

inline derp_isp_config parse_isp_config(const std::string& text) {
  derp_isp_config k;
  derp_isp_config_default(&k);
  JsonParser jp(text);
  const Json root = jp.value();
  jp.ws();
  if (root.kind != Json::Obj || jp.p != text.size()) {
    LOG_FATAL("isp JSON: the file must hold one object");
  }
  const Json* cam = root.find("CameraIsp");
  if (!cam || cam->kind == Json::Null) {
    LOG_WARNING("Missing \"CameraIsp\" in config; using default values.");
    return k;
  }
  if (cam->kind != Json::Obj) {
    LOG_FATAL("isp JSON: \"CameraIsp\" must be an object");
  }
  auto integer = [&](const char* key, int32_t& out) {
    if (const Json* j = cam->find(key)) {
      out = (int32_t)isp_number(*j, key);
    }
  };
  auto real = [&](const char* key, float& out) {
    if (const Json* j = cam->find(key)) {
      out = (float)isp_number(*j, key);
    }
  };
  auto boolean = [&](const char* key, int32_t& out) {  // folly asBool: a bool, or a number != 0
    if (const Json* j = cam->find(key)) {
      if (j->kind != Json::Bool && j->kind != Json::Num) {
        LOG_FATAL(std::string("isp JSON: '") + key + "' must be true or false");
      }
      out = j->kind == Json::Bool ? j->boolean : j->num != 0;
    }
  };
  auto word = [&](const char* key, char (&out)[8], bool mayBeEmpty) {  // upper case, four letters
    if (const Json* j = cam->find(key)) {
      if (j->kind != Json::Str || !(j->str.size() == 4 || (mayBeEmpty && j->str.empty()))) {
        LOG_FATAL(std::string("isp JSON: '") + key + "' must be a string of four letters");
      }
      memset(out, 0, sizeof out);
      for (size_t i = 0; i < j->str.size(); ++i) {
        out[i] = (char)toupper((unsigned char)j->str[i]);
      }
    }
  };
  integer("bitsPerPixel", k.bits_per_pixel);
  integer("width", k.width);
  integer("height", k.height);
  boolean("isLittleEndian", k.is_little_endian);
  boolean("isRowMajor", k.is_row_major);
  word("bayerPattern", k.bayer_pattern, false);
  word("planeOrder", k.plane_order, true);
  const int nLut = isp_points(*cam, "compandingLut", nullptr, 0);  // parsed and, as in the reference, never used
  if (nLut >= 0) {
    k.n_companding_lut = nLut;
  }
  isp_point(*cam, "blackLevel", k.black_level);
  isp_point(*cam, "clampMin", k.clamp_min);
  isp_point(*cam, "clampMax", k.clamp_max);
  integer("stuckPixelThreshold", k.stuck_pixel_threshold);
  CHECK_MSG(k.stuck_pixel_threshold >= 0, "stuckPixelThreshold");
  real("stuckPixelDarknessThreshold", k.stuck_pixel_darkness_threshold);
  integer("stuckPixelRadius", k.stuck_pixel_radius);
  const int nH = isp_points(*cam, "vignetteRollOffH", k.rolloff_h, DERP_ISP_MAX_ROLLOFF);
  const int nV = isp_points(*cam, "vignetteRollOffV", k.rolloff_v, DERP_ISP_MAX_ROLLOFF);
  if (nH >= 0) {
    k.n_rolloff_h = nH;
  }
  if (nV >= 0) {
    k.n_rolloff_v = nV;
  }
  isp_point(*cam, "whiteBalanceGain", k.white_balance_gain);
  if (const Json* m = cam->find("ccm"); m && m->kind != Json::Null) {  // getMatrix (:456-478); 3 x 3 is what setup() uses
    if (m->kind != Json::Arr || m->arr.size() != 3) {
      LOG_FATAL("isp JSON: 'ccm' must be a 3 x 3 matrix");
    }
    for (int r = 0; r < 3; ++r) {
      if (m->arr[r].kind != Json::Arr || m->arr[r].arr.size() != 3) {
        LOG_FATAL("isp JSON: 'ccm' must be a 3 x 3 matrix");
      }
      for (int c = 0; c < 3; ++c) {
        k.ccm[3 * r + c] = (float)isp_number(m->arr[r].arr[c], "ccm");
      }
    }
  }
  real("saturation", k.saturation);
  isp_point(*cam, "gamma", k.gamma);
  isp_point(*cam, "lowKeyBoost", k.low_key_boost);
  isp_point(*cam, "highKeyBoost", k.high_key_boost);
  real("contrast", k.contrast);
  isp_point(*cam, "sharpening", k.sharpening);
  real("sharpeningSupport", k.sharpening_support);
  real("noiseCore", k.noise_core);
  return k;
}

// cameraIspFromConfigFileWithOptions (RawUtil.cpp:47-49)
inline derp_isp_config load_isp_config(const fs::path& path) {
  const std::string text = read_file_or_empty(path);
  CHECK_MSG(!text.empty(), "could not read JSON file: " + path.string());
  return parse_isp_config(text);
}

}  // namespace cli
